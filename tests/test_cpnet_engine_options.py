"""CPnetEngineOptions: the BE_CPNET_* variables parsed once, and an engine built from explicit options
equal to the one built under the same environment."""
import pytest
import torch

from bioengine_worker_amd.models.cpnet import CPnet, CPnetEngine, CPnetEngineOptions
from bioengine_worker_amd.ops import conv as cv

VARS = ("BE_CPNET_PAIR", "BE_CPNET_PAIR_LEVELS", "BE_CPNET_IGEMM", "BE_CPNET_IGEMM_LEVELS", "BE_CPNET_HEAD",
        "BE_CPNET_PP_CFG")

# (environment, the same as explicit options)
SETTINGS = {
    "default": ({}, CPnetEngineOptions()),
    "pair_off": ({"BE_CPNET_PAIR": "0"}, CPnetEngineOptions(pair=False)),
    "igemm_off": ({"BE_CPNET_IGEMM": "0"}, CPnetEngineOptions(igemm="0")),
    "pp_23": ({"BE_CPNET_IGEMM": "pp", "BE_CPNET_IGEMM_LEVELS": "2,3"}, CPnetEngineOptions(igemm="pp", igemm_levels=(2, 3))),
    "pair_level_0": ({"BE_CPNET_PAIR_LEVELS": "0"}, CPnetEngineOptions(pair_levels=(0,))),
    "igemm_levels_empty": ({"BE_CPNET_IGEMM_LEVELS": ""}, CPnetEngineOptions(igemm_levels=None)),
}


@pytest.fixture
def clean_env(monkeypatch):
    for v in VARS:
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def net():
    return CPnet().randomize_(0)


def test_defaults(clean_env):
    opt = CPnetEngineOptions.from_env()
    assert opt == CPnetEngineOptions()
    assert opt.pair is True and opt.pair_levels == (0, 1) and opt.igemm == "1" and opt.igemm_levels == (3,)
    assert opt.head is True and opt.pp_cfg is None


@pytest.mark.parametrize("name", list(SETTINGS))
def test_engine_from_options_equals_engine_from_environment(clean_env, net, name):
    env, opt = SETTINGS[name]
    for k, v in env.items():
        clean_env.setenv(k, v)
    assert CPnetEngineOptions.from_env() == opt
    by_env = CPnetEngine(net, "cpu")
    for k in env:
        clean_env.delenv(k)
    by_opt = CPnetEngine(net, "cpu", opt)
    assert set(by_env.pair) == set(by_opt.pair) and set(by_env.ig) == set(by_opt.ig)
    assert (by_env.head is None) == (by_opt.head is None)
    # 32 x 32 is the smallest input with a pixel at level 3
    x = torch.randn(1, 32, 32, by_env.cin_pad, generator=torch.Generator().manual_seed(1)).bfloat16()
    x[..., 2:] = 0
    (ya, sa), (yb, sb) = by_env(x), by_opt(x)
    assert torch.equal(ya, yb) and torch.equal(sa, sb)


def test_pp128_build_names_the_ping_pong_layers_of_the_default_plan(clean_env, net):
    eng = CPnetEngine(net, "cpu")
    named = {}
    for side, blocks in (("down", eng.down), ("up", eng.up)):
        for lv, e in enumerate(blocks):
            for k in ("proj", "c0", "c1", "c2", "c3"):
                build = cv.pp128_build(e[k].pc)
                if build is not None:
                    named[(side, lv, k)] = build
    assert cv.pp128_build(eng.out.pc) is None
    # level 2: its 128 -> 128 3x3 convs (down c1..c3; every 3x3 of up block 2 but c0, which reads 256
    # channels), its entry conv and projection; level 3: its entry conv
    want = {("down", 2, k): "c128" for k in ("c1", "c2", "c3")}
    want.update({("up", 2, k): "c128" for k in ("c1", "c2", "c3")})
    want.update({("down", 2, "c0"): "pool", ("down", 2, "proj"): "proj", ("down", 3, "c0"): "c256"})
    assert named == want
