"""float16 DeepQN without a GPU: DeepQNHalf's initialisation, dtypes, accessors, checkpoints and mutation against the
reference's float16 fixture (tests/golden/deepqn_forward_f16.json) and torch, the C checker (tests/dqn16_checker.py) against
the reference's logits and on its edges, and the float16 slab and workspace sizes (the symbols of the float16 DeepQN ABI:
tests/test_abi.py)."""
import hashlib

import numpy as np
import pytest
import torch

from coevonet_amd import game_logic as gl
from coevonet_amd import lib as L
from coevonet_amd.atari_synthetic import SyntheticAtariAEC
from coevonet_amd.deepqn import PARAM_ORDER, DeepQN, DeepQNHalf
from oracle import ref_port as rp
from tests import dqn16_checker as ck
from tests.util import DQN_FRAME_KINDS, Bag, dqn_golden_frames, load_golden, sha

# the largest |checker - reference| over the 48 fixture rows, in fp16 ulps of the row's largest |logit| (measured, see
# test_checker_vs_reference_fixture), and the bound the test asserts: that maximum plus one ulp
MEASURED_ULPS = 4.25
BOUND_ULPS = MEASURED_ULPS + 1.0


def fixture_net(c, mutated=True):
    torch.manual_seed(c["torch_seed"])
    net = DeepQNHalf(c["C"], c["n_actions"], "float16")
    if mutated:
        for p in net.parameters():
            p.data += torch.normal(0, c["mutate_std"], size=p.size())
    return net


def atari_env(C=4):
    env = SyntheticAtariAEC("pong_v3", channels=C)
    env.reset(seed=1)
    return env


def offsets(C, n):
    """start of every parameter in the canonical flat order"""
    shapes = [(32, C, 8, 8), (32,), (64, 32, 4, 4), (64,), (64, 64, 3, 3), (64,), (512, 3136), (512,), (n, 512), (n,),
              (32,), (32,), (64,), (64,), (64,), (64,)]
    off, out = 0, {}
    for k, s in zip(PARAM_ORDER, shapes):
        out[k] = (off, int(np.prod(s)))
        off += int(np.prod(s))
    assert off == rp.lib().oracle_dqn_param_count(C, n)
    return out


def test_initial_and_mutated_weights_are_the_reference_half_weights():
    for c in load_golden("deepqn_forward_f16.json")["cases"]:
        assert sha(fixture_net(c, mutated=False).flat()) == c["init_sha256"], c["torch_seed"]
        net = fixture_net(c)
        assert sha(net.flat()) == c["weights_sha256"], c["torch_seed"]
        assert {k: str(v.dtype).replace("torch.", "") for k, v in net.state_dict().items()} == c["dtypes"]
        frames = dqn_golden_frames(c["C"], c["frame_pcg_seed"])
        assert hashlib.sha256(frames.tobytes()).hexdigest() == c["frame_sha256"]


def test_create_agent_and_clone_draw_like_the_float32_agent():
    env = atari_env()
    states = {}
    for prec in ("float32", "float16"):
        args = Bag(game="pong_v3", precision=prec)
        torch.manual_seed(21)
        a = gl.create_agent(env, args)
        after_create = torch.random.get_rng_state()
        a.mutate(0.02)
        b = a.clone(env, args)
        states[prec] = (after_create, torch.random.get_rng_state(), a, b)
    assert torch.equal(states["float32"][0], states["float16"][0])
    assert torch.equal(states["float32"][1], states["float16"][1])
    _, _, a, b = states["float16"]
    assert isinstance(a.model, DeepQNHalf) and isinstance(b.model, DeepQNHalf) and not isinstance(a.model, DeepQN)
    assert isinstance(states["float32"][2].model, DeepQN)
    for k, v in a.model.state_dict().items():
        w = b.model.state_dict()[k]
        assert w.dtype == v.dtype and torch.equal(w, v), k
    # the half agent starts from the float32 agent's draws, rounded once
    torch.manual_seed(21)
    f32 = gl.create_agent(env, Bag(game="pong_v3", precision="float32")).model.flat()
    torch.manual_seed(21)
    f16 = gl.create_agent(env, Bag(game="pong_v3", precision="float16")).model.flat()
    assert np.array_equal(f16, f32.astype(np.float16).astype(np.float32))


def test_mutate_is_the_reference_half_update():
    """Agent.mutate on a float16 Atari agent == f16(f32(parent) + noise) for EVERY parameter, the BatchNorm affine included,
    with the global generator's draws in parameters() order - torch's own half_param.data += torch.normal(...)"""
    env = atari_env()
    torch.manual_seed(11)
    a = gl.create_agent(env, Bag(game="pong_v3", precision="float16"))
    parents = {k: v.clone() for k, v in zip(PARAM_ORDER, a.model.parameters())}
    state = torch.random.get_rng_state()
    a.mutate(0.3)
    torch.random.set_rng_state(state)
    for k, got in zip(PARAM_ORDER, a.model.parameters()):
        noise = torch.normal(0, 0.3, size=parents[k].size()).numpy()
        want = (parents[k].numpy().astype(np.float32) + noise).astype(np.float16)
        assert got.dtype == torch.float16 and np.array_equal(got.numpy().view(np.uint16), want.view(np.uint16)), k


class TorchHalfDeepQN(torch.nn.Module):
    """a half torch.nn module of the reference's structure (registration order of Atari/deepqn.py:16-37), built here"""

    def __init__(self, C, n):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(C, 32, kernel_size=8, stride=4)
        self.conv2 = torch.nn.Conv2d(32, 64, kernel_size=4, stride=2)
        self.conv3 = torch.nn.Conv2d(64, 64, kernel_size=3, stride=1)
        self.fc1 = torch.nn.Linear(64 * 7 * 7, 512)
        self.output = torch.nn.Linear(512, n)
        self.vbn1 = torch.nn.BatchNorm2d(32)
        self.vbn2 = torch.nn.BatchNorm2d(64)
        self.vbn3 = torch.nn.BatchNorm2d(64)
        self.to(torch.float16)


def test_state_dict_round_trip_with_a_half_torch_module(tmp_path):
    from coevonet_amd.io_utils import agents_from_state_dicts, save_state_dicts
    c = load_golden("deepqn_forward_f16.json")["cases"][0]
    net = fixture_net(c)
    sd = net.state_dict()
    assert all(v.dtype == (torch.long if k.endswith("num_batches_tracked") else torch.float16) for k, v in sd.items())
    mod = TorchHalfDeepQN(c["C"], c["n_actions"])
    assert list(mod.state_dict().keys()) == list(sd.keys())
    mod.load_state_dict(sd, strict=True)
    for k, v in mod.state_dict().items():
        assert v.dtype == sd[k].dtype and torch.equal(v, sd[k]), k
    torch.manual_seed(77)
    other = DeepQNHalf(c["C"], c["n_actions"], "float16")
    assert sha(other.flat()) != sha(net.flat())
    other.load_state_dict(mod.state_dict(), strict=True)
    assert sha(other.flat()) == c["weights_sha256"]
    with pytest.raises(KeyError):
        other.load_state_dict({k: v for k, v in sd.items() if k != "fc1.bias"}, strict=True)
    # get_weights / set_weights and the flat accessors keep half values
    w = net.get_weights(["vbn1"])
    assert set(w) == {"vbn1.weight", "vbn1.bias", "vbn1.running_mean", "vbn1.running_var", "vbn1.num_batches_tracked"}
    other.set_flat(np.zeros_like(net.flat()))
    other.set_flat(net.flat())
    assert sha(other.flat()) == c["weights_sha256"]
    # the weights_only-safe checkpoint carries a half Atari agent
    env = atari_env(c["C"])
    args = Bag(game="pong_v3", precision="float16")
    torch.manual_seed(5)
    ags = [gl.create_agent(env, args) for _ in range(2)]
    for a in ags:
        a.mutate(0.05)
    path = save_state_dicts(ags, str(tmp_path / "pop.pth"), role="first_0")
    back = agents_from_state_dicts(env, args, None, path)
    for a, b in zip(ags, back):
        assert isinstance(b.model, DeepQNHalf)
        for k, v in a.model.state_dict().items():
            assert b.model.state_dict()[k].dtype == v.dtype and torch.equal(b.model.state_dict()[k], v)


def test_pickle_checkpoints_carry_the_half_agent(tmp_path):
    """save_model -> load_agent_for_testing (the pickles main.py --test reads): GA files are Hall-of-Fame lists whose newest
    member is taken, ES files single agents; the half nets come back with their dtypes and values"""
    from coevonet_amd.io_utils import load_agent_for_testing, save_model
    env = atari_env()
    args = Bag(game="pong_v3", precision="float16")
    torch.manual_seed(8)
    ags = [gl.create_agent(env, args) for _ in range(3)]
    for a in ags:
        a.mutate(0.05)
    paths = [str(tmp_path / f"a{i}.pth") for i in range(3)]
    for a, p in zip(ags, paths):
        save_model(a, p)
    es = load_agent_for_testing(Bag(algorithm="ES", ES_model_to_test_agent_0=paths[0], ES_model_to_test_agent_1=paths[1],
                                    ES_model_to_test_adversary_0=paths[2]))
    for a, p in zip(ags, paths):
        save_model([ags[0], a], p)
    gaa = load_agent_for_testing(Bag(algorithm="GA", GA_hof_to_test_agent_0=paths[0], GA_hof_to_test_agent_1=paths[1],
                                     GA_hof_to_test_adversary=paths[2]))
    for back in (es, gaa):
        for a, b in zip(ags, back):
            assert isinstance(b.model, DeepQNHalf) and b.precision == "float16"
            for k, v in a.model.state_dict().items():
                w = b.model.state_dict()[k]
                assert w.dtype == v.dtype and torch.equal(w, v), k


def test_es_accessors_round_trip_on_half_values():
    c = load_golden("deepqn_forward_f16.json")["cases"][2]
    net = fixture_net(c)
    args = Bag(precision="float16")
    allw = net.get_weights_ES()
    assert allw.dtype == np.float16 and allw.size == rp.lib().oracle_dqn_param_count(c["C"], c["n_actions"])
    assert np.array_equal(allw.astype(np.float32), net.flat())   # all eight layers = the canonical flat order
    pw = net.get_perturbable_weights()
    assert pw.dtype == np.float16 and pw.size == allw.size - 320   # no BatchNorm affine
    bn_before = [net._params[k].clone() for k in PARAM_ORDER[-6:]]
    g = np.random.default_rng(1)
    new = (pw.astype(np.float32) + g.normal(0, 0.01, pw.size).astype(np.float32)).astype(np.float16)   # half values
    net.set_perturbable_weights(new, args)
    assert np.array_equal(net.get_perturbable_weights().view(np.uint16), new.view(np.uint16))
    # what is not a half value goes through the reference's own conversion, torch.tensor(slice, dtype=torch.float16)
    wide = new.astype(np.float64) + g.normal(0, 1e-4, pw.size)
    net.set_perturbable_weights(wide, args)
    assert np.array_equal(net.get_perturbable_weights(), torch.tensor(wide, dtype=torch.float16).numpy())
    net.set_perturbable_weights(new, args)
    assert all(torch.equal(a, net._params[k]) for a, k in zip(bn_before, PARAM_ORDER[-6:]))
    net.set_weights_ES(allw, args, net.layers)
    assert sha(net.flat()) == c["weights_sha256"]


def test_checker_rounding_is_numpy_float16():
    rng = np.random.default_rng(0)
    x = (rng.normal(0, 1, 2000) * 10.0 ** rng.integers(-9, 6, 2000)).astype(np.float32)
    edges = np.array([65504, 65519.996, 65520, 1e9, -65520, 6e-8, 2.9802322e-08, 2.9802326e-08, 6.1e-5, 6.0975552e-05,
                      1.0009765625, 1.00048828125, 1.00146484375, 0.0, -0.0, np.inf, -np.inf], dtype=np.float32)
    x = np.concatenate([x, edges])
    with np.errstate(over="ignore"):
        want = x.astype(np.float16).view(np.uint16)
    assert np.array_equal(ck.f16_bits(x), want)


def test_checker_vs_reference_fixture():
    """The reference's torch-CPU half conv2d / Linear do not accumulate in the canonical order, so this is a measured bound:
    over the 48 fixture rows the largest |checker - reference| is 4.25 fp16 ulps of the row's largest |logit| (measured on
    the build machine with torch 2.10; 32 rows are at or below 1 ulp); the test asserts that maximum plus one ulp, 5.25.  Actions
    are compared on the rows whose reference top-2 margin exceeds twice that bound: 47 of the 48 rows (the fixture's mutate
    std 0.02 leaves one row with a margin of 2.8 ulps), and all 47 have the reference's action."""
    worst, qualifying, equal = 0.0, 0, 0
    for c in load_golden("deepqn_forward_f16.json")["cases"]:
        net = fixture_net(c)
        frames = dqn_golden_frames(c["C"], c["frame_pcg_seed"])
        for r in range(len(DQN_FRAME_KINDS)):
            a, lg, st = ck.forward(net.flat(), c["C"], c["n_actions"], frames[r])
            ref = np.array(c["logits"][r])
            u = ck.ulp16(np.max(np.abs(ref)))
            d = np.max(np.abs(lg.astype(np.float64) - ref)) / u
            print(c["torch_seed"], DQN_FRAME_KINDS[r], "ulps", d)
            worst = max(worst, d)
            assert st == 0
            assert np.array_equal(lg, lg.astype(np.float16).astype(np.float32))   # fp16 values
            srt = np.sort(ref)[::-1]
            if srt[0] - srt[1] > 2 * BOUND_ULPS * u:
                qualifying += 1
                equal += int(a == int(np.argmax(ref)))
    print("largest distance", worst, "ulps; qualifying", qualifying, "equal", equal)
    assert worst <= BOUND_ULPS
    assert qualifying >= 36            # at least three quarters of the 48 rows
    assert (qualifying, equal) == (47, 47)


def small_net(C=4, n=6, seed=3):
    torch.manual_seed(seed)
    return ck.half_net(C, n)


def test_checker_conv_overflow_gives_nan_logits_and_no_action():
    C, n = 4, 6
    net = small_net(C, n)
    off = offsets(C, n)
    o, m = off["conv1.weight"]
    net[o:o + m] = 60000.0                                    # an fp16 value; 256 taps of x = 1 pass 65504
    frame = np.full((84, 84, C), 255, dtype=np.uint8)
    a, lg, st = ck.forward(net, C, n, frame)
    assert np.isnan(lg).all() and st == ck.ST_NO_ACTION and a == 0


def test_checker_zero_variance_frame():
    """all-0 frame: every conv1 sum of a channel is f16(bias), the strided sums of 400 equal fp16 values are exact, so the mean
    is that value, d = 0, var = 0 and the BatchNorm output is beta whatever conv1's bias and vbn1's gamma are"""
    C, n = 4, 6
    net = small_net(C, n)
    off = offsets(C, n)
    frame = np.zeros((84, 84, C), dtype=np.uint8)
    a0, lg0, st0 = ck.forward(net, C, n, frame)
    assert st0 == 0 and np.isfinite(lg0).all()
    other = net.copy()
    o, m = off["conv1.bias"]
    other[o:o + m] = np.linspace(-3, 3, m).astype(np.float16)
    o, m = off["vbn1.weight"]
    other[o:o + m] = np.linspace(-50, 50, m).astype(np.float16)
    a1, lg1, st1 = ck.forward(other, C, n, frame)
    assert st1 == 0 and a1 == a0 and np.array_equal(lg0.view(np.uint32), lg1.view(np.uint32))
    # ... and on a frame with variance the same change does move the logits
    g = np.random.Generator(np.random.PCG64(5))
    fr = g.integers(0, 256, size=(84, 84, C), dtype=np.uint8)
    assert not np.array_equal(ck.forward(net, C, n, fr)[1], ck.forward(other, C, n, fr)[1])


def test_checker_exact_tie_takes_the_first_index():
    C, n = 4, 6
    net = small_net(C, n)
    off = offsets(C, n)
    o, m = off["output.weight"]
    net[o:o + m] = 0.0
    o, m = off["output.bias"]
    net[o:o + m] = np.array([0.125, 0.25, 0.5, 0.375, 0.5, 0.125], dtype=np.float32)
    g = np.random.Generator(np.random.PCG64(6))
    a, lg, st = ck.forward(net, C, n, g.integers(0, 256, size=(84, 84, C), dtype=np.uint8))
    assert st == 0 and lg[2] == lg[4] == 0.5 and a == 2


def test_dqn16_slab_stride_and_workspace_sizes():
    """(the entry points in the header, the library and the binding: tests/test_abi.py)"""
    from coevonet_amd.build import build
    build()
    lib = L.load()
    assert lib.coevo_version() == 103
    # the slab: a multiple of 4 words, about 0.52 of the fp32 slab; bad shapes are argument errors
    assert lib.coevo_dqn16_slab_stride(4, 6) == (884710 + 63) // 64 * 64
    for C, n in ((1, 1), (3, 6), (6, 18), (6, 32)):
        assert lib.coevo_dqn16_slab_stride(C, n) % 4 == 0
    for C, n in ((0, 6), (7, 6), (4, 0), (4, 33), (4 | L.DQN_FC1_TILED, 6)):
        assert lib.coevo_dqn16_slab_stride(C, n) == -1
    assert lib.coevo_dqn16_workspace_bytes(0) == -1 and lib.coevo_dqn16_workspace_bytes(3) == 3 * (3136 + 512) * 4
    import coevonet_amd
    assert coevonet_amd.DeepQNHalf is DeepQNHalf


def test_deepqnhalf_refuses_other_precisions_before_the_library_is_loaded(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded before the precision was checked")
    monkeypatch.setattr(L, "load", no_load)
    for prec in ("float32", "bfloat16", None):
        with pytest.raises(ValueError):
            DeepQNHalf(4, 6, prec)


def test_pinned_refusals_still_hold():
    from tests.test_fp16_cpu import test_out_of_scope_float16_combinations_raise
    test_out_of_scope_float16_combinations_raise()
    with pytest.raises(ValueError):
        DeepQN(4, 6, "float16")
