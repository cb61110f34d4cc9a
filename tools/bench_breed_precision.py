"""float32 against float16 breeding launches of ONE cfg 2-shaped generation, from the same elites:

    python tools/bench_breed_precision.py [--repeats 9] [--warmup 3] [--settle-ms 120] [--out profiles/r08_fp16_breeding.md]

3 roles x 199 children from E = 2 elites (pop 200), stale-agent distances fused in.  float32: ONE coevo_fc_perturb_dist_multi
launch + ONE coevo_fc_distance_finalize_multi (what GAEngine enqueues per cohort).  float16: per role coevo_fc16_perturb_dist
+ coevo_fc16_distance_finalize (what HalfGAEngine.breed enqueues: six launches).  The elites' Linear entries are fp16 values,
so both precisions breed from the same nets with the same noise streams.  After the warm-up the two variants alternate
(untimed) until --settle-ms of work has passed, then alternate for --repeats timed rounds each (device events around the
variant's launches); the table has medians and the min .. max spread.  Run it as one GPU step under its own time limit."""
import argparse
import ctypes as ct
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from coevonet_amd import lib as L                   # noqa: E402
from tools.bench_precision import ROLE_D, ROLES, random_flat   # noqa: E402

DEV = "cuda"


def build(precision, flats, pop, E):
    """-> dict(run = enqueue the variant's launches, bytes written per call, tensors kept alive)"""
    half = precision == "float16"
    stride = {r: (L.fc16_slab_stride if half else L.fc_slab_stride)(ROLE_D[r]) for r in ROLES}
    nb = {r: (L.fc16_perturb_blocks(ROLE_D[r]) if half else int(L.load().coevo_fc_perturb_blocks(ROLE_D[r]))) for r in ROLES}
    keep = {"slab": {}, "part": {}, "dist": {}, "head": {}, "sigma": {}}
    idx = torch.tensor([c % E for c in range(pop - 1)], dtype=torch.int32, device=DEV)
    for r in ROLES:   # per role [elite E | stale 1 | pop]
        slab = torch.zeros((E + 1 + pop) * stride[r], dtype=torch.int32 if half else torch.float32, device=DEV)
        src = torch.from_numpy(flats[r]).to(DEV)
        L.call("coevo_fc16_pack" if half else "coevo_fc_pack", L._p(src), L._p(slab), E + 1, ROLE_D[r])
        keep["slab"][r] = slab
        keep["part"][r] = torch.zeros((pop - 1) * nb[r], dtype=torch.float64, device=DEV)
        keep["dist"][r] = torch.zeros(pop, dtype=torch.float32, device=DEV)
        keep["head"][r] = torch.zeros(1, dtype=torch.float32, device=DEV)
        keep["sigma"][r] = torch.full((1,), 0.05, dtype=torch.float32, device=DEV)
    at = lambda r, net: keep["slab"][r].data_ptr() + 4 * net * stride[r]   # noqa: E731

    if half:
        def run():
            for ri, r in enumerate(ROLES):
                L.call("coevo_fc16_perturb_dist", at(r, 0), L._p(idx), at(r, E + 1), 1, pop - 1, ROLE_D[r], L._p(keep["sigma"][r]),
                       0, 0, ri, 0, None, at(r, E), L._p(keep["part"][r]))
                L.call("coevo_fc16_distance_finalize", L._p(keep["part"][r]), nb[r], pop - 1, L._p(keep["dist"][r]), 1,
                       L._p(keep["head"][r]))
    else:
        pj, fj = (L.PerturbJob * 3)(), (L.FinalizeJob * 3)()
        for ri, r in enumerate(ROLES):
            pj[ri] = L.PerturbJob(at(r, 0), L._p(idx), at(r, E + 1), L._p(keep["sigma"][r]), at(r, E), L._p(keep["part"][r]), 1,
                                  pop - 1, ROLE_D[r], 0, ri, 0)
            fj[ri] = L.FinalizeJob(L._p(keep["part"][r]), L._p(keep["dist"][r]), L._p(keep["head"][r]), nb[r], pop - 1, 1, 0)

        def run():
            L.call("coevo_fc_perturb_dist_multi", ct.cast(pj, ct.c_void_p), 3, 0, 0, None)
            L.call("coevo_fc_distance_finalize_multi", ct.cast(fj, ct.c_void_p), 3)
    return {"name": precision, "run": run, "keep": (keep, idx), "ms": [],
            "bytes": sum(4 * stride[r] * (pop - 1) for r in ROLES), "dist": keep["dist"]}


def one(v, timed):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    v["run"]()
    e1.record()
    e1.synchronize()
    if timed:
        v["ms"].append(e0.elapsed_time(e1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, default=200)
    ap.add_argument("--elites", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=120.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r08_fp16_breeding.md"))
    a = ap.parse_args()
    assert a.repeats >= 5, "at least 5 repeats of each variant"
    rng = np.random.default_rng(8)
    flats = {r: np.stack([random_flat(rng, ROLE_D[r]) for _ in range(a.elites + 1)]) for r in ROLES}
    variants = [build(p, flats, a.pop, a.elites) for p in ("float32", "float16")]
    for _ in range(a.warmup):
        for v in variants:
            one(v, False)
    t0, settle = time.perf_counter(), 0
    while (time.perf_counter() - t0) * 1e3 < a.settle_ms:
        for v in variants:
            one(v, False)
        settle += 1
    for _ in range(a.repeats):
        for v in variants:   # alternating: a drift of the clocks lands on both alike
            one(v, True)
    d32 = np.concatenate([variants[0]["dist"][r].cpu().numpy()[1:] for r in ROLES])
    d16 = np.concatenate([variants[1]["dist"][r].cpu().numpy()[1:] for r in ROLES])
    rel = float(np.max(np.abs(d16 - d32) / d32))
    lines = [f"# float32 vs float16 breeding launches, cfg 2 shape ({torch.cuda.get_device_name(0)})", "",
             f"3 roles x {a.pop - 1} children from {a.elites} elites, stale-agent distances fused in; float32 = one "
             "coevo_fc_perturb_dist_multi + one coevo_fc_distance_finalize_multi launch, float16 = three coevo_fc16_perturb_dist + "
             f"three coevo_fc16_distance_finalize launches; warm-up {a.warmup}, {settle} settling rounds ({a.settle_ms:.0f} ms), "
             f"{a.repeats} alternating timed repeats of each variant.", "",
             "| variant | child MB written | median ms | min .. max ms | median GB/s written |", "|---|---|---|---|---|"]
    for v in variants:
        ms = np.array(v["ms"])
        med = float(np.median(ms))
        lines.append(f"| {v['name']} | {v['bytes'] / 1e6:.1f} | {med:.4f} | {ms.min():.4f} .. {ms.max():.4f} | "
                     f"{v['bytes'] / med / 1e6:.0f} |")
    m32, m16 = (float(np.median(v["ms"])) for v in variants)
    lines += ["", f"fp16 median / fp32 median: {m16 / m32:.3f}",
              f"largest relative difference between the fp16 and the fp32 children's distances: {rel:.2e} "
              "(the fp16 children are the rounded fp32 children)"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
