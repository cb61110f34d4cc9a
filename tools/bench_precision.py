"""float32 against float16 device rollout of ONE cfg 2-shaped batch, from the same random nets:

    python tools/bench_precision.py [--repeats 7] [--warmup 3] [--settle-ms 120] [--out profiles/r07_fp16_rollout.md]

3 roles x pop 200, HoF 5 -> 3000 games, 2 cohorts (contiguous individuals), 25 env-cycles, 16-row shared-opponent tasks: the
task tables GAEngine builds (without its 10 evaluation games).  The Linear entries of the nets are fp16 values, so both
precisions play the same nets.  Variants: the fp32 rollout (default cache-resident budget) and the fp16 rollout under three
cache policies - no task resident, the default budget, every task resident.  After the warm-up the variants alternate
(untimed) until --settle-ms of work has passed, as bench.py's settling steps do, then alternate for --repeats timed
rollouts each (device events around reset + rollout); the table has medians and the min .. max spread.  Run it as one GPU
step under its own time limit, e.g.  timeout -k 10 300 python tools/bench_precision.py && <the next step>."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from coevonet_amd import genetic_algorithm as ga   # noqa: E402
from coevonet_amd import lib as L                   # noqa: E402
from coevonet_amd.fcnetwork import LINEAR_KEYS, param_shapes   # noqa: E402
from coevonet_amd.rollout import DeviceRollout, RolloutPlan    # noqa: E402

DEV = "cuda"
ROLES = ("agent_0", "agent_1", "adversary_0")
ROLE_D = {"agent_0": 10, "agent_1": 10, "adversary_0": 8}


def random_flat(rng, D):
    """torch-like init magnitudes, Linear entries rounded to fp16, LayerNorm affine near (1, 0)"""
    flat = rng.uniform(-0.3, 0.3, L.fc_param_count(D)).astype(np.float32)
    off = 0
    for k, s in param_shapes(D):
        n = int(np.prod(s))
        if k.startswith("ln"):
            flat[off:off + n] = np.float32(1.0 if k.endswith("weight") else 0.0) + rng.normal(0, 0.05, n).astype(np.float32)
        elif k in LINEAR_KEYS:
            flat[off:off + n] = flat[off:off + n].astype(np.float16).astype(np.float32)
        off += n
    return flat


def build(pop, hof, K, seed):
    """-> games (adversary, agent_0, agent_1 net ids), game cohorts, per net id (role, region, index), flats per role"""
    ids, nets = {}, []

    def net(region, role, i):
        if (region, role, i) not in ids:
            ids[(region, role, i)] = len(nets)
            nets.append((role, region, i))
        return ids[(region, role, i)]

    games, h = [], hof
    for role in ROLES:
        for i in range(pop):
            for k in range(h):   # the seats GAEngine fills (genetic_algorithm.py:136-142, :168-174, :201-207 of the reference)
                if role == "agent_0":
                    a0, a1, adv = net("pop", role, i), net("hof", "agent_1", h - 1 - k), net("hof", "adversary_0", h - 1 - k)
                elif role == "agent_1":
                    a0, a1, adv = net("hof", "agent_0", h - 1 - k), net("pop", role, i), net("hof", "adversary_0", h - 1 - k)
                else:
                    a0, a1, adv = net("hof", "agent_0", h - 1 - k), net("hof", "agent_0", h - 1 - k), net("pop", role, i)
                games.append((adv, a0, a1))
    bounds, per = ga.cohort_partition(pop, K)
    per_ind = np.repeat(per, hof)
    cohort = np.concatenate([per_ind, per_ind, per_ind]).astype(np.int32)
    rng = np.random.default_rng(seed)
    flats = {r: np.stack([random_flat(rng, ROLE_D[r]) for _ in range(pop + hof)]) for r in ROLES}
    return games, cohort, nets, flats, bounds


def make_variant(precision, policy, games, cohort, nets, flats, bounds, pop, hof):
    stride = {r: (L.fc16_slab_stride if precision == "float16" else L.fc_slab_stride)(ROLE_D[r]) for r in ROLES}
    base, at = {}, 0
    for r in ROLES:
        base[r] = at
        at += (pop + hof) * stride[r]
    slab = torch.zeros(at, dtype=torch.int32 if precision == "float16" else torch.float32, device=DEV)
    for r in ROLES:
        src = torch.from_numpy(flats[r]).to(DEV)
        L.call("coevo_fc16_pack" if precision == "float16" else "coevo_fc_pack", L._p(src), slab.data_ptr() + 4 * base[r],
               pop + hof, ROLE_D[r])
    where = lambda role, region, i: base[role] + ((i if region == "pop" else pop + i) * stride[role])   # noqa: E731
    net_off = [where(*n) for n in nets]
    net_D = [ROLE_D[n[0]] for n in nets]
    ind_bytes = sum(4 * stride[r] for r in ROLES)
    K = len(bounds) - 1
    budget = {"none": 0.0, "default": ga.RESIDENT_MB_DEFAULT * 1e6, "all": float("inf")}[policy]
    n_res = ga.resident_prefix(budget, (hof + 1) * ind_bytes, ind_bytes, bounds)   # the Hall of Fame and the stale trio count
    res = [j for j, (role, region, i) in enumerate(nets) if region == "pop" and
           any(bounds[k] <= i < bounds[k] + int(n_res[k]) for k in range(K))]
    plan = RolloutPlan(np.array(games), net_off, net_D, device=DEV, heavy_rows=16, game_cohort=cohort, resident_nets=res)
    ro = DeviceRollout(plan, slab, precision=precision)
    distinct = {int(t["net_off"]): 4 * stride["adversary_0" if int(t["D"]) == 8 else "agent_0"]
                for arr in (plan.heavy_np, plan.light_np) for t in arr}
    return {"name": f"{precision} / {policy}", "ro": ro, "plan": plan, "bytes": sum(distinct.values()),
            "resident_tasks": int((plan.light_np["reserved"] & L.TASK_RESIDENT).sum()), "light": len(plan.light_np),
            "heavy": len(plan.heavy_np), "ms": []}


def one(v, n_cycles, timed):
    ro = v["ro"]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ro.reset(0, ro.plan.n_games, 1)
    ro.run(n_cycles)
    e1.record()
    e1.synchronize()
    if timed:
        v["ms"].append(e0.elapsed_time(e1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, default=200)
    ap.add_argument("--hof", type=int, default=5)
    ap.add_argument("--cohorts", type=int, default=2)
    ap.add_argument("--cycles", type=int, default=25)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=120.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r07_fp16_rollout.md"))
    a = ap.parse_args()
    assert a.repeats >= 5, "at least 5 repeats of each variant"
    games, cohort, nets, flats, bounds = build(a.pop, a.hof, a.cohorts, seed=7)
    variants = [make_variant(p, pol, games, cohort, nets, flats, bounds, a.pop, a.hof)
                for p, pol in (("float32", "default"), ("float16", "none"), ("float16", "default"), ("float16", "all"))]
    T = 3 * a.cycles
    for v in variants:
        v["ro"].set_limits([T] * len(games))
    for _ in range(a.warmup):
        for v in variants:
            one(v, a.cycles, False)
    t0, settle = time.perf_counter(), 0
    while (time.perf_counter() - t0) * 1e3 < a.settle_ms:
        for v in variants:
            one(v, a.cycles, False)
        settle += 1
    for _ in range(a.repeats):
        for v in variants:   # alternating: a drift of the clocks lands on every variant alike
            one(v, a.cycles, True)
    for v in variants:
        v["ro"].check_status()
    rew = [v["ro"].rewards.cpu().numpy() for v in variants]
    same16 = all(np.array_equal(rew[1].view(np.uint64), r.view(np.uint64)) for r in rew[2:])
    lines = [f"# float32 vs float16 device rollout, cfg 2 shape ({torch.cuda.get_device_name(0)})", "",
             f"{len(games)} games, {a.cohorts} cohorts, {a.cycles} env-cycles, pop {a.pop} x 3 roles, HoF {a.hof}; one rollout = reset + "
             f"{a.cycles} cycle launches per cohort + the closing step, replayed as a graph; warm-up {a.warmup}, {settle} settling "
             f"rounds ({a.settle_ms:.0f} ms), {a.repeats} alternating timed repeats of each variant.", "",
             "| variant | tasks (heavy + light) | resident tasks | weight MB / cycle | median ms | min .. max ms | median GB/s of weights |",
             "|---|---|---|---|---|---|---|"]
    for v in variants:
        ms = np.array(v["ms"])
        med = float(np.median(ms))
        lines.append(f"| {v['name']} | {v['heavy']} + {v['light']} | {v['resident_tasks']} | {v['bytes'] / 1e6:.1f} | {med:.3f} | "
                     f"{ms.min():.3f} .. {ms.max():.3f} | {v['bytes'] * a.cycles / med / 1e6:.0f} |")
    m32 = float(np.median(variants[0]["ms"]))
    lines += ["", "fp16 median / fp32 median: " + ", ".join(f"{v['name']} {float(np.median(v['ms'])) / m32:.3f}" for v in variants[1:]),
              f"rewards of the three fp16 cache policies bit-identical: {same16}"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    if not same16:
        raise SystemExit("the fp16 cache policies disagree")


if __name__ == "__main__":
    main()
