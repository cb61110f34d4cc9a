#!/usr/bin/env python3
"""float32 against float16 DeepQN forward on the agent-step task tables of cfg 4 and cfg 5, from the same random nets:

    python tools/bench_dqn_precision.py [--shapes cfg4,cfg5] [--repeats 15] [--warmup 3] [--settle-ms 120] [--out FILE.md]

The task tables are those of tools/bench_dqn_shapes.py (cfg 4: 50 population nets x 10 games + 10 Hall-of-Fame nets x 50 / 60
games in 16-row tasks; cfg 5: one cohort, 125 perturbed nets x 1 game + the base net x 125 games).  Every parameter of the
nets is an fp16 value, so both precisions run the same nets: the fp32 forward (coevo_dqn_forward_argmax, streamed fc1 layout)
on an fp32 slab, the fp16 forward (coevo_dqn16_forward_argmax) on an fp16 slab, in one process.  After the warm-up the two
alternate (untimed) until --settle-ms of work has passed, then alternate for --repeats timed forwards each (device events
around the three launches); the table has medians and the min .. max spread.  The per-kernel split (conv launch, fc1, output
layer) comes from a run of its own under  rocprofv3 --kernel-trace --stats -- python tools/bench_dqn_precision.py --repeats 7.
Run it as one GPU step under its own time limit."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from coevonet_amd import lib as L   # noqa: E402

DEV = "cuda"
ROWS = L.DQN_MAX_ROWS


def cut(rows):
    return [min(ROWS, rows - i) for i in range(0, rows, ROWS)]


def table(shape):
    """-> (n_actions, n_nets, [(net, rows)]) as tools/bench_dqn_shapes.py builds them"""
    if shape == "cfg4":
        layout = [(i, 10) for i in range(50)]
        for j in range(10):
            layout += [(50 + j, r) for r in (cut(60) if j == 0 else cut(50))]
        return 6, 60, layout
    if shape == "cfg5":
        layout = [(1 + j, 1) for j in range(125)] + [(0, r) for r in cut(125)]
        return 18, 126, layout
    raise SystemExit(f"unknown shape {shape}")


class Variant:
    def __init__(self, precision, flat, layout, C, n_act, frames):
        lib = L.load()
        self.name, self.sym = precision, "coevo_dqn16" if precision == "float16" else "coevo_dqn"
        n_nets = flat.shape[0]
        self.stride = int(getattr(lib, self.sym + "_slab_stride")(C, n_act))
        self.slab = torch.zeros(n_nets, self.stride, dtype=torch.int32 if precision == "float16" else torch.float32, device=DEV)
        L.call(self.sym + "_pack", L._p(flat), L._p(self.slab), n_nets, C, n_act)
        tasks = np.zeros(len(layout), dtype=L.DQN_TASK_DTYPE)
        row = 0
        for i, (net, r) in enumerate(layout):
            tasks[i] = (net * self.stride, row, r)
            row += r
        self.rows, self.n_tasks, self.C, self.n_act, self.frames = row, len(layout), C, n_act, frames
        self.tasks = L.tasks_to_device(tasks, DEV)
        self.actions = torch.zeros(row, dtype=torch.int32, device=DEV)
        self.status = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.ws = torch.zeros(int(getattr(lib, self.sym + "_workspace_bytes")(row)) // 4, dtype=torch.float32, device=DEV)
        self.fn = getattr(lib, self.sym + "_forward_argmax")
        self.stream = torch.cuda.current_stream().cuda_stream
        self.us = []

    def run(self, timed=False):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L._check(self.fn(L._p(self.slab), L._p(self.tasks), self.n_tasks, ROWS, self.rows, self.C, self.n_act,
                         L._p(self.frames), L._p(self.actions), None, L._p(self.status), L._p(self.ws), self.stream), self.sym)
        e1.record()
        e1.synchronize()
        if timed:
            self.us.append(e0.elapsed_time(e1) * 1e3)


def measure(shape, C, a):
    n_act, n_nets, layout = table(shape)
    P = int(L.load().coevo_dqn_param_count(C, n_act))
    g = torch.Generator(device=DEV).manual_seed(7)
    flat = torch.randn(n_nets, P, device=DEV, generator=g) * 0.02
    for lo, hi in ((P - 320, P - 288), (P - 256, P - 192), (P - 128, P - 64)):   # vbn*.weight near 1
        flat[:, lo:hi] += 1.0
    flat = flat.to(torch.float16).to(torch.float32).contiguous()
    rows = sum(r for _, r in layout)
    frames = torch.randint(0, 256, (rows, 84, 84, C), dtype=torch.uint8, device=DEV, generator=g)
    vs = [Variant(p, flat, layout, C, n_act, frames) for p in ("float32", "float16")]
    del flat
    for _ in range(a.warmup):
        for v in vs:
            v.run()
    t0, settle = time.perf_counter(), 0
    while (time.perf_counter() - t0) * 1e3 < a.settle_ms:
        for v in vs:
            v.run()
        settle += 1
    for _ in range(a.repeats):
        for v in vs:   # alternating: a drift of the clocks lands on both alike
            v.run(True)
    for v in vs:
        assert int(v.status.item()) == 0, f"{v.name}: status {int(v.status.item())}"
    equal = float((vs[0].actions == vs[1].actions).float().mean().item())   # the two precisions act alike on most rows, not all
    lines = [f"## {shape}: {rows} rows, {len(layout)} tasks, {n_nets} nets, C = {C}, {n_act} actions", "",
             f"warm-up {a.warmup}, {settle} settling rounds ({a.settle_ms:.0f} ms), {a.repeats} alternating timed repeats", "",
             "| variant | slab bytes / net | weight MB of the launch | median us | min .. max us | status |", "|---|---|---|---|---|---|"]
    for v in vs:
        us = np.array(v.us)
        lines.append(f"| {v.name} | {4 * v.stride} | {4 * v.stride * n_nets / 1e6:.1f} | {np.median(us):.1f} | "
                     f"{us.min():.1f} .. {us.max():.1f} | {int(v.status.item())} |")
    m32, m16 = (float(np.median(v.us)) for v in vs)
    lines += ["", f"fp16 median / fp32 median: {m16 / m32:.3f}; slab bytes fp16 / fp32: {vs[1].stride / vs[0].stride:.3f}; "
              f"rows with equal actions: {equal:.3f}", ""]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg4,cfg5")
    ap.add_argument("--C", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=120.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 7, "at least 7 repeats of each variant"
    lines = [f"# float32 vs float16 DeepQN forward ({torch.cuda.get_device_name(0)})", ""]
    for shape in a.shapes.split(","):
        lines += measure(shape, a.C, a)
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
