#!/usr/bin/env python3
"""Mint tests/golden/ppo_baseline.npz from the REFERENCE's three trained PPO policies (PPO/model_{agent_0,agent_1,
adversary_0}.pth) and its own PPOPolicy class, imported from the reference tree and never copied.  Run in the build container
only:

    python tests/golden/make_golden_ppo.py

What is recorded, per role (data only - weights and recorded results; no checkpoint pickle, no reference source):
  <role>.flat        the policy weights as raw float32 in MLPBaseline's flat order (the value head is not carried)
  <role>.obs         N_STORED observations, the first rows of 4096 uniform(-2, 2) rows drawn from numpy's default_rng(SEED)
  <role>.logits      torch's logits (PPOPolicy.forward) for them
  <role>.actions     PPOPolicy.get_action_and_value(obs, deterministic=True) actions for them
  <role>.max_dlogit  max |torch logit - exact restatement (tests/checker16/mlp_checker.c)| over ALL 4096 rows
  <role>.stats       over all 4096 rows: [rows whose top-two margin in the checker is below 8 max_dlogit, action mismatches
                     among the other rows, rows where argmax(softmax) differs from the first maximum]
4096 rows per role with their logits would be 3 x 4096 x (10 + 5) x 4 bytes - past the size of the largest existing fixture
(114 KB) beside the 61 KB of weights - so N_STORED = 256 rows per role are stored; the statistics still cover all 4096.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from PPO.PPOagent import PPOPolicy  # noqa: E402

from coevonet_amd.baselines import MLPBaseline  # noqa: E402
from tests import baseline_cases as bc  # noqa: E402

SEED, N_ALL, N_STORED = 0, 4096, 256


def main():
    torch.set_num_threads(1)
    out = {"seed": np.int64(SEED), "n_all": np.int64(N_ALL)}
    for r, role in enumerate(bc.ROLES):
        D = bc.ROLE_D[role]
        sd = torch.load(os.path.join(REF, "PPO", f"model_{role}.pth"), map_location="cpu", weights_only=True)
        policy = PPOPolicy(D, 5)
        policy.load_state_dict(sd)
        policy.eval()
        base = MLPBaseline.from_state_dict(sd)
        obs = np.random.default_rng(SEED + r).uniform(-2, 2, size=(N_ALL, D)).astype(np.float32)
        with torch.no_grad():
            logits = policy.forward(torch.from_numpy(obs))[0].numpy().astype(np.float32)
            soft = torch.argmax(torch.softmax(torch.from_numpy(logits), dim=-1), dim=-1).numpy()
            actions = np.array([policy.get_action_and_value(torch.from_numpy(o), deterministic=True)[0] for o in obs[:N_STORED]],
                               dtype=np.int32)
        ck_actions, ck_logits, st = bc.mlp_rows(base.flat, D, obs)
        assert not st.any()
        dmax = float(np.abs(logits.astype(np.float64) - ck_logits.astype(np.float64)).max())
        top = np.sort(ck_logits.astype(np.float64), axis=1)
        clear = top[:, -1] - top[:, -2] >= 8 * dmax
        torch_first_max = np.argmax(logits, axis=1)   # (np.argmax returns the first maximum)
        stats = np.array([int((~clear).sum()), int((ck_actions[clear] != torch_first_max[clear]).sum()),
                          int((soft != torch_first_max).sum())], dtype=np.int64)
        assert np.array_equal(actions, soft[:N_STORED])
        print(f"{role}: max |dlogit| {dmax:.3e}, below the margin {stats[0]} of {N_ALL} ({100.0 * stats[0] / N_ALL:.3f} %), "
              f"mismatches {stats[1]}, argmax(softmax) != first max {stats[2]}")
        out[f"{role}.flat"] = base.flat
        out[f"{role}.obs"] = obs[:N_STORED]
        out[f"{role}.logits"] = logits[:N_STORED]
        out[f"{role}.actions"] = actions
        out[f"{role}.max_dlogit"] = np.float64(dmax)
        out[f"{role}.stats"] = stats
    path = os.path.join(HERE, "ppo_baseline.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
