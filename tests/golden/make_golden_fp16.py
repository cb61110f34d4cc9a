#!/usr/bin/env python3
"""Mint the float16 fixtures by running the REFERENCE's own Python with ``precision="float16"`` (imported from the
reference checkout, never copied) against this repo's AEC env.  Build container only:

    python tests/golden/make_golden_fp16.py         # writes tests/golden/*_f16.json

  fc_forward_f16.json  FCNetwork(D, 5, "float16").forward / determine_action on seeded nets (fresh and GA-mutated, the
                       mutation being the reference's own ``half_param.data += torch.normal(...)``) + observations
  play_game_f16.json   play_game() with float16 agents: reward triples, every forward's action, top logit and top-2 margin

Every forward records its top-2 margin (in fp16 logits) so that tests know which actions a 1-ulp logit difference could
flip.  The environment shims and helpers are make_golden.py's (imported, not edited).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402  (puts the reference and the repo on sys.path, shims supersuit)

FCNetwork = mg.FCNetwork


class ForwardLog:
    def __init__(self):
        self.cur = None

    def begin(self):
        self.cur = {"actions": [], "margins": [], "tops": []}


LOG = ForwardLog()


def _logged_forward(self, x, args):
    out = mg._orig_forward(self, x, args)
    if LOG.cur is not None:
        o = out.detach().to(torch.float64).numpy()
        srt = np.sort(o)[::-1]
        LOG.cur["margins"].append(float(srt[0] - srt[1]))
        LOG.cur["tops"].append(float(srt[0]))
        LOG.cur["actions"].append(int(np.argmax(o)))   # first maximum, as determine_action's strict '>' scan
    return out


FCNetwork.forward = _logged_forward


def mutate_half(net, std):
    """agent.py:25-29 on the half net: every parameter += N(0, std) drawn in parameters() order"""
    for p in net.parameters():
        p.data += torch.normal(0, std, size=p.size())


def mint_fc_forward_f16():
    args = mg.Bag(precision="float16")
    cases = []
    for seed, D in [(0, 10), (1, 8), (2, 10), (3, 8), (4, 10), (5, 8)]:
        torch.manual_seed(seed)
        net = FCNetwork(D, 5, "float16")
        if seed >= 2:
            mutate_half(net, 0.05)
        g = np.random.Generator(np.random.PCG64(300 + seed))
        obs = g.uniform(-2, 2, size=(16, D)).astype(np.float32)
        logits, actions, margins = [], [], []
        for r in range(obs.shape[0]):
            x = torch.from_numpy(obs[r]).to(torch.float16)   # preprocess_observation (utils/game_logic_functions.py:69-72)
            out = mg._orig_forward(net, x, args)
            o = out.detach().to(torch.float64).numpy()
            srt = np.sort(o)[::-1]
            logits.append([float(v) for v in o])
            margins.append(float(srt[0] - srt[1]))
            actions.append(int(net.determine_action(x, args)))
        sd = net.state_dict()
        cases.append({"torch_seed": seed, "mutated": seed >= 2, "mutate_std": 0.05, "D": D, "obs": obs.tolist(),
                      "logits": logits, "actions": actions, "margins": margins, "weights": mg.wsum(net),
                      "dtypes": {k: str(v.dtype).replace("torch.", "") for k, v in sd.items()}})
    mg.dump("fc_forward_f16.json", {"cases": cases})


def mint_play_game_f16():
    out = []
    for seed, limit, max_cycles, mutated in [(10, None, 25, False), (11, 50, 25, False), (12, 200, 70, False),
                                             (13, 7, 25, False), (14, None, 25, True), (15, 120, 70, True)]:
        mg.seed_all(seed)
        env = mg.make_env(max_cycles)
        args = mg.Bag(max_timesteps_per_episode=limit, max_evaluation_steps=limit, precision="float16")
        a0 = mg.ref_glf.create_agent(env, args, "agent_0")
        a1 = mg.ref_glf.create_agent(env, args, "agent_1")
        adv = mg.ref_glf.create_agent(env, args, "adversary_0")
        if mutated:
            for a in (a0, a1, adv):
                a.mutate(0.05)
        games = []
        for _ in range(3):
            LOG.begin()
            ret = mg._orig_play_game(env=env, player1=a0.model, player2=a1.model, adversary=adv.model, args=args,
                                     eval=False)
            g = LOG.cur
            LOG.cur = None
            g["rewards"] = [float(x) for x in ret]
            g["steps"] = len(g["actions"])
            g["min_margin"] = min(g["margins"])
            games.append(g)
        out.append({"torch_seed": seed, "limit": limit, "max_cycles": max_cycles, "mutated": mutated,
                    "mutate_std": 0.05, "weights": [mg.wsum(a0.model), mg.wsum(a1.model), mg.wsum(adv.model)],
                    "games": games})
    mg.dump("play_game_f16.json", {"cases": out})


if __name__ == "__main__":
    which = set(sys.argv[1:])
    if not which or "fc" in which:
        mint_fc_forward_f16()
    if not which or "play" in which:
        mint_play_game_f16()
