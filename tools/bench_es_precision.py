"""float32 against float16 Co-ES update and perturb launches of ONE cfg 3-shaped generation:

    python tools/bench_es_precision.py [--pop 1000] [--repeats 9] [--warmup 3] [--settle-ms 120] [--out FILE]

3 roles x pop 1000.  update float32: per role coevo_es_partial + coevo_es_apply (what ESEngine.update_device enqueues: the
partial launch streams the materialised perturbed nets).  update float16: per role coevo_es16_fitness + coevo_es16_partial +
coevo_es16_apply (what HalfESEngine.update enqueues: the partial launch draws every individual's noise again and reads no
net).  perturb float32: per role coevo_fc_perturb_flags; perturb float16: per role coevo_fc16_perturb_dist, both with LayerNorm
untouched and no distances.  The fitness has zero mean, so repeated updates do not feed on themselves.  After the warm-up the
four variants alternate (untimed) until --settle-ms of work has passed, then alternate for --repeats timed rounds each (device
events around the variant's launches); the table has medians and the min .. max spread.  --once NAME enqueues one variant a
few times without timing (for a kernel trace).  Run it as one GPU step under its own time limit."""
import argparse
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
CHUNKS = 8
RET_SLOT = {"agent_0": 0, "agent_1": 1, "adversary_0": 2}


def build(flats, pop, sigma=0.05, lr=0.1):
    """-> {variant name: enqueue function}, tensors kept alive"""
    keep = []
    zero_idx = torch.zeros(pop, dtype=torch.int32, device=DEV)
    rng = np.random.default_rng(9)
    rewards = rng.normal(0.0, 20.0, (3 * pop, 3))
    rewards -= rewards.mean(axis=0)
    rew = torch.from_numpy(rewards).to(DEV)
    per_role = {}
    for ri, r in enumerate(ROLES):
        D = ROLE_D[r]
        s32, s16 = L.fc_slab_stride(D), L.fc16_slab_stride(D)
        slab32 = torch.zeros((1 + pop) * s32, dtype=torch.float32, device=DEV)
        slab16 = torch.zeros((1 + pop) * s16, dtype=torch.int32, device=DEV)
        src = torch.from_numpy(flats[r][None]).to(DEV)
        L.call("coevo_fc_pack", L._p(src), L._p(slab32), 1, D)
        L.call("coevo_fc16_pack", L._p(src), L._p(slab16), 1, D)
        game_idx = (torch.arange(pop, dtype=torch.int32, device=DEV) * 3 + ri).contiguous()
        fit32 = rew[game_idx.long(), RET_SLOT[r]].to(torch.float32).contiguous()
        per_role[r] = dict(D=D, ri=ri, s32=s32, s16=s16, slab32=slab32, slab16=slab16, game_idx=game_idx, fit32=fit32,
                           fit16=torch.zeros(pop, dtype=torch.float32, device=DEV),
                           part32=torch.zeros(CHUNKS * s32, dtype=torch.float32, device=DEV),
                           part16=torch.zeros(CHUNKS * L.es16_partial_floats(D), dtype=torch.float32, device=DEV),
                           sigma=torch.full((1,), sigma, dtype=torch.float32, device=DEV))
    keep += [zero_idx, rew, per_role, src]

    def perturb32():
        for r in ROLES:
            q = per_role[r]
            L.call("coevo_fc_perturb_flags", L._p(q["slab32"]), L._p(zero_idx), q["slab32"].data_ptr() + 4 * q["s32"], 0, pop,
                   q["D"], L._p(q["sigma"]), 0, 0, q["ri"], 1)

    def perturb16():
        for r in ROLES:
            q = per_role[r]
            L.call("coevo_fc16_perturb_dist", L._p(q["slab16"]), L._p(zero_idx), q["slab16"].data_ptr() + 4 * q["s16"], 0, pop,
                   q["D"], L._p(q["sigma"]), 0, 0, q["ri"], 1, None, None, None)

    def update32():
        for r in ROLES:
            q = per_role[r]
            L.call("coevo_es_partial", L._p(q["slab32"]), q["slab32"].data_ptr() + 4 * q["s32"], 0, q["D"], L._p(q["fit32"]), pop,
                   CHUNKS, 0, CHUNKS, L._p(q["part32"]))
            L.call("coevo_es_apply", L._p(q["slab32"]), L._p(q["part32"]), CHUNKS, CHUNKS, CHUNKS * q["s32"], q["D"], pop,
                   L._p(q["sigma"]), L.C.c_float(lr))

    def update16():
        for r in ROLES:
            q = per_role[r]
            L.call("coevo_es16_fitness", L._p(rew), L._p(q["game_idx"]), RET_SLOT[r], pop, None, L._p(q["fit16"]))
            L.call("coevo_es16_partial", q["D"], L._p(q["fit16"]), pop, CHUNKS, L._p(q["sigma"]), 0, 0, q["ri"], L._p(q["part16"]))
            L.call("coevo_es16_apply", L._p(q["slab16"]), L._p(q["part16"]), CHUNKS, q["D"], pop, L._p(q["sigma"]), lr)

    variants = [("perturb float32", perturb32), ("perturb float16", perturb16), ("update float32", update32),
                ("update float16", update16)]
    return [{"name": n, "run": f, "ms": []} for n, f in variants], keep


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
    ap.add_argument("--pop", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=120.0)
    ap.add_argument("--once", default=None, help="enqueue this variant three times, untimed, and exit")
    ap.add_argument("--out", default=None, help="also write the table to this file (profiles/r09_fp16_es.md holds one run)")
    a = ap.parse_args()
    rng = np.random.default_rng(8)
    flats = {r: random_flat(rng, ROLE_D[r]) for r in ROLES}
    variants, keep = build(flats, a.pop)
    if a.once:
        v = [v for v in variants if v["name"] == a.once][0]
        variants[0]["run"](), variants[1]["run"]()
        for _ in range(3):
            v["run"]()
        torch.cuda.synchronize()
        return
    assert a.repeats >= 5, "at least 5 repeats of each variant"
    for _ in range(a.warmup):
        for v in variants:
            one(v, False)
    t0, settle = time.perf_counter(), 0
    while (time.perf_counter() - t0) * 1e3 < a.settle_ms:
        for v in variants:
            one(v, False)
        settle += 1
    for _ in range(a.repeats):
        for v in variants:   # alternating: a drift of the clocks lands on all alike
            one(v, True)
    lines = [f"# float32 vs float16 Co-ES perturb and update launches, cfg 3 shape ({torch.cuda.get_device_name(0)})", "",
             f"3 roles x pop {a.pop}, {CHUNKS} update chunks; perturb = three launches (LayerNorm untouched, no distances); update "
             "float32 = three coevo_es_partial + three coevo_es_apply, update float16 = three coevo_es16_fitness + three "
             f"coevo_es16_partial + three coevo_es16_apply; warm-up {a.warmup}, {settle} settling rounds ({a.settle_ms:.0f} ms), "
             f"{a.repeats} alternating timed repeats of each variant.", "",
             "| variant | median ms | min .. max ms |", "|---|---|---|"]
    for v in variants:
        ms = np.array(v["ms"])
        lines.append(f"| {v['name']} | {float(np.median(ms)):.4f} | {ms.min():.4f} .. {ms.max():.4f} |")
    med = {v["name"]: float(np.median(v["ms"])) for v in variants}
    lines += ["", f"update float16 / update float32: {med['update float16'] / med['update float32']:.3f}",
              f"update float16 / perturb float16: {med['update float16'] / med['perturb float16']:.3f}",
              f"perturb float16 / perturb float32: {med['perturb float16'] / med['perturb float32']:.3f}"]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
