#!/usr/bin/env python3
"""Mint the float16 DeepQN fixture by running the REFERENCE's own ``DeepQN(C, n, "float16")`` on the CPU (imported from
the reference checkout, never copied).  Build container only:

    python tests/golden/make_golden_dqn_fp16.py         # writes tests/golden/deepqn_forward_f16.json

  deepqn_forward_f16.json  six seeded half nets (C = 3, 4, 5, 6 planes, 6 / 18 actions), mutated with the reference's own
                           ``half_param.data += torch.normal(0, std, size)`` over every parameter, on the eight frames of
                           tests/util.dqn_golden_frames: the reference's half logits, the sha256 of the initial and the
                           mutated weights (their float32 image in parameters() order, as tests/util.sha hashes) and of
                           the frames

The helpers are make_golden.py's (imported, not edited).  MUTATE_STD is chosen so that at least three quarters of the rows
have a top-2 margin the checker's measured distance to the reference cannot flip (tests/test_fp16_dqn_cpu.py).
"""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402  (puts the reference and the repo on sys.path)

DeepQN = mg.DeepQN
MUTATE_STD = 0.02
CASES = [(0, 4, 6), (1, 6, 18), (2, 3, 6), (3, 5, 18), (4, 4, 18), (5, 6, 6)]


def flat32(net):
    """the parameters in state_dict order (= parameters() order: the BatchNorm affine last) as float32"""
    sd = net.state_dict()
    return np.concatenate([sd[k].detach().numpy().ravel() for k in sd
                           if not k.endswith("num_batches_tracked") and "running" not in k]).astype(np.float32)


def mint(std=MUTATE_STD):
    from tests.util import DQN_FRAME_KINDS, dqn_golden_frames
    cases = []
    for seed, C, n in CASES:
        torch.manual_seed(seed)
        net = DeepQN(C, n, "float16")
        init_sha = hashlib.sha256(flat32(net).tobytes()).hexdigest()
        for p in net.parameters():   # agent.py:25-29 on the half net
            p.data += torch.normal(0, std, size=p.size())
        frames = dqn_golden_frames(C, 200 + seed)
        logits = []
        for r in range(frames.shape[0]):
            # preprocess_observation (utils/game_logic_functions.py:76-80): HWC uint8 -> [1, C, 84, 84]; forward casts to half
            x = torch.from_numpy(frames[r]).permute(2, 0, 1).unsqueeze(0)
            out = net.forward(x)
            assert out.dtype == torch.float16
            logits.append([float(v) for v in out.detach().to(torch.float64).numpy()[0]])
        sd = net.state_dict()
        cases.append({"torch_seed": seed, "C": C, "n_actions": n, "frame_pcg_seed": 200 + seed,
                      "frame_kinds": DQN_FRAME_KINDS, "frame_sha256": hashlib.sha256(frames.tobytes()).hexdigest(),
                      "mutate_std": std, "init_sha256": init_sha,
                      "weights_sha256": hashlib.sha256(flat32(net).tobytes()).hexdigest(), "logits": logits,
                      "dtypes": {k: str(v.dtype).replace("torch.", "") for k, v in sd.items()}})
    return {"cases": cases}


if __name__ == "__main__":
    mg.dump("deepqn_forward_f16.json", mint())
