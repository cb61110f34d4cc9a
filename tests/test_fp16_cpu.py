"""float16 nets without a GPU: the half net's initialisation, dtypes, checkpoints and mutation against the reference's
float16 fixtures (tests/golden/*_f16.json) and torch, the C checker against the reference, and the refusals of what
float16 does not cover."""
import numpy as np
import pytest
import torch

from coevonet_amd import game_logic as gl
from coevonet_amd.fcnetwork import FCNetwork, FCNetworkHalf, LINEAR_KEYS
from coevonet_amd.mpe.simple_adversary import ENV_SEED, SimpleAdversaryAEC
from oracle import ref_port as rp
from tests import fp16_checker as ck
from tests.util import Bag, load_golden, sha

ROLES = ("agent_0", "agent_1", "adversary_0")


def fixture_net(c):
    torch.manual_seed(c["torch_seed"])
    net = FCNetworkHalf(c["D"], 5)
    if c["mutated"]:
        for p in net.parameters():
            p.data += torch.normal(0, c["mutate_std"], size=p.size())
    return net


def fixture_agents(c):
    torch.manual_seed(c["torch_seed"])
    np.random.seed(c["torch_seed"])
    env = SimpleAdversaryAEC(max_cycles=c["max_cycles"])
    env.reset(seed=ENV_SEED)
    args = Bag(precision="float16", max_timesteps_per_episode=c["limit"], max_evaluation_steps=c["limit"])
    ags = [gl.create_agent(env, args, r) for r in ROLES]
    if c["mutated"]:
        for a in ags:
            a.mutate(c["mutate_std"])
    return env, args, ags


def test_create_agent_float16_draws_like_the_reference():
    for c in load_golden("fc_forward_f16.json")["cases"]:
        assert sha(fixture_net(c).flat()) == c["weights"]["sha256"], c["torch_seed"]
    for c in load_golden("play_game_f16.json")["cases"]:
        _, _, ags = fixture_agents(c)
        assert all(isinstance(a.model, FCNetworkHalf) for a in ags)
        assert [sha(a.model.flat()) for a in ags] == [w["sha256"] for w in c["weights"]], c["torch_seed"]


def test_state_dict_dtypes_and_checkpoint_round_trip(tmp_path):
    from coevonet_amd.io_utils import agents_from_state_dicts, save_state_dicts
    c = load_golden("fc_forward_f16.json")["cases"][0]
    net = fixture_net(c)
    sd = net.state_dict()
    assert {k: str(v.dtype).replace("torch.", "") for k, v in sd.items()} == c["dtypes"]
    assert all((v.dtype == torch.float16) == (k in LINEAR_KEYS) for k, v in sd.items())
    assert net.get_weights_ES().dtype == np.float16   # the reference concatenates the half tensors' numpy views
    env = SimpleAdversaryAEC()
    env.reset(seed=ENV_SEED)
    args = Bag(precision="float16")
    torch.manual_seed(5)
    ags = [gl.create_agent(env, args, "agent_0") for _ in range(2)]
    for a in ags:
        a.mutate(0.1)
    path = save_state_dicts(ags, str(tmp_path / "pop.pth"), role="agent_0")
    back = agents_from_state_dicts(env, args, "agent_0", path)
    for a, b in zip(ags, back):
        assert isinstance(b.model, FCNetworkHalf)
        for k, v in a.model.state_dict().items():
            w = b.model.state_dict()[k]
            assert w.dtype == v.dtype and torch.equal(w, v)
    # clone keeps dtypes and values
    cl = ags[0].clone(env, args, "agent_0")
    assert sha(cl.model.flat()) == sha(ags[0].model.flat())


def test_mutate_is_the_reference_half_update():
    """Agent.mutate on a float16 agent == f16(f32(parent) + noise) on Linear entries, parent + noise on LayerNorm entries,
    with the global generator's draws in parameters() order - torch's own half_param.data += torch.normal(...)"""
    env = SimpleAdversaryAEC()
    env.reset(seed=ENV_SEED)
    args = Bag(precision="float16")
    torch.manual_seed(11)
    a = gl.create_agent(env, args, "adversary_0")
    parents = {k: v.clone() for k, v in a.model.state_dict().items()}
    state = torch.random.get_rng_state()
    a.mutate(0.3)
    torch.random.set_rng_state(state)
    for k, p in parents.items():
        noise = torch.normal(0, 0.3, size=p.size()).numpy()
        if k in LINEAR_KEYS:
            want = (p.numpy().astype(np.float32) + noise).astype(np.float16)
        else:
            want = p.numpy() + noise
        got = a.model.state_dict()[k].numpy()
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8)), k


def test_preprocess_observation_float16():
    obs = np.array([0.1, -1.5, 70000.0], dtype=np.float32)
    x = gl.preprocess_observation(obs, Bag(precision="float16"))
    assert x.dtype == torch.float16 and torch.isinf(x[2])
    assert gl.preprocess_observation(obs, Bag(precision="float32")).dtype == torch.float32


def test_checker_rounding_is_numpy_float16():
    rng = np.random.default_rng(0)
    x = (rng.normal(0, 1, 4000) * 10.0 ** rng.integers(-9, 6, 4000)).astype(np.float32)
    edges = np.array([65504, 65519.996, 65520, 1e9, -65520, 6e-8, 2.9802322e-08, 2.9802326e-08, 6.1e-5, 6.0975552e-05,
                      0.0, -0.0, np.inf, -np.inf], dtype=np.float32)
    x = np.concatenate([x, edges])
    with np.errstate(over="ignore"):
        want = x.astype(np.float16).view(np.uint16)
    assert np.array_equal(ck.f16_bits(x), want)


def test_checker_forward_vs_reference_fixture():
    """logits within one fp16 ulp of the row's largest |logit| (not of each logit: the reference's torch-CPU half Linear does
    not accumulate in the canonical order, so a logit near zero can differ by many of its own ulps); actions equal wherever
    the reference's margin exceeds two ulps of its top logit - which every one of the 96 fixture rows does"""
    safe = 0
    for c in load_golden("fc_forward_f16.json")["cases"]:
        net = fixture_net(c)
        for obs, ref, ref_a, m in zip(c["obs"], c["logits"], c["actions"], c["margins"]):
            a, lg, st = ck.forward(net.flat(), c["D"], obs)
            assert st == 0
            assert np.max(np.abs(lg.astype(np.float64) - np.array(ref))) <= ck.ulp16(np.max(np.abs(ref)))
            if m > 2 * ck.ulp16(max(ref)):
                assert a == ref_a
                safe += 1
    assert safe == 96


def test_checker_play_game_vs_reference_fixture():
    """every one of the 18 fixture games - exact logit ties included - has the reference's actions and rewards"""
    exact = 0
    for c in load_golden("play_game_f16.json")["cases"]:
        _, _, ags = fixture_agents(c)
        stream = rp.Stream()
        for gi, g in enumerate(c["games"]):
            got = ck.play_game(stream, *[a.model.flat() for a in ags], c["limit"], c["max_cycles"])
            assert got["status"] == 0 and got["steps"] == g["steps"]
            assert got["actions"] == g["actions"], (c["torch_seed"], gi)
            assert got["rewards"] == g["rewards"], (c["torch_seed"], gi)
            exact += 1
    assert exact == 18


def test_out_of_scope_float16_combinations_raise():
    from coevonet_amd import evolutionary_strategy as es
    from coevonet_amd import genetic_algorithm as ga
    from coevonet_amd.deepqn import DeepQN
    env = SimpleAdversaryAEC()
    env.reset(seed=ENV_SEED)
    args = Bag(precision="float16", population=4, hof_size=1, generations=1, max_timesteps_per_episode=6,
               max_evaluation_steps=6)
    with pytest.raises(ValueError, match="Co-GA training with precision float16"):
        ga.genetic_algorithm_train(env, None, args, None)
    with pytest.raises(ValueError, match="Co-GA training with precision float16"):
        ga.genetic_algorithm_train(env, None, args, None, rng="device_philox", env_mode="host")
    with pytest.raises(ValueError, match="Co-ES with precision float16"):
        es.evolution_strategy_train(env, Bag(algorithm="ES", precision="float16", population=4), None)
    with pytest.raises(ValueError):
        DeepQN(4, 6, "float16")
    with pytest.raises(ValueError):
        FCNetwork(10, 5, "float16")
    with pytest.raises(ValueError):
        FCNetworkHalf(10, 5, "float32")
    with pytest.raises(ValueError):
        gl.preprocess_observation(np.zeros(3, dtype=np.float32), Bag(precision="bfloat16"))
