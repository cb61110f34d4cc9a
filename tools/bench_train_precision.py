"""The float16 trainers measured: the breeding launches of one generation as per-role launches against the multi launches,
and a whole float16 trainer step against the float32 trainer's, Co-GA at the cfg 2 shape and Co-ES at the cfg 3 shape:

    python tools/bench_train_precision.py [--repeats 9] [--warmup 3] [--settle-ms 120] [--out profiles/r19_fp16_trainers.md]

Breeding, Co-GA (pop 200, E 2): 3 roles x 199 children with their stale-agent distances as three coevo_fc16_perturb_dist +
three coevo_fc16_distance_finalize launches (HalfGAEngine's default) against one coevo_fc16_perturb_dist_multi + one
coevo_fc16_distance_finalize_multi (``multi_breed=True``, what GATrainer builds).  Co-ES (pop 1000, no fitness sharing): the
3 x 1000 perturbed nets as three launches against one.  Device events around the variant's launches.
Steps: ``GATrainer.step`` (pop 200, hof 5, E 2, T 200, collect=False) with precision float16 (host-driven loop) against float32
in its default host-free device loop, and ``ESTrainer.step`` (pop 1000) likewise; rng device_philox, device env; the host
clock around step() + a device synchronize.
Every pair: warm-up, the two variants alternating (untimed) until --settle-ms have passed, then --repeats alternating timed
rounds each; the tables have medians and the min .. max spread.  Run it as one GPU step under its own time limit."""
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
from coevonet_amd.game_logic import initialize_env  # noqa: E402
from tools.bench_precision import ROLE_D, ROLES, random_flat   # noqa: E402

DEV = "cuda"


def breed_variants(flats, n, parents, with_dist, flags):
    """-> the per-role and the multi variant over ONE set of fp16 slabs: per role [parents | reference 1 | n children]"""
    stride = {r: L.fc16_slab_stride(ROLE_D[r]) for r in ROLES}
    nb = {r: L.fc16_perturb_blocks(ROLE_D[r]) for r in ROLES}
    keep = {"slab": {}, "part": {}, "dist": {}, "head": {}, "sigma": {}}
    idx = torch.tensor([c % parents for c in range(n)], dtype=torch.int32, device=DEV)
    for r in ROLES:
        slab = torch.zeros((parents + 1 + n) * stride[r], dtype=torch.int32, device=DEV)
        L.call("coevo_fc16_pack", L._p(torch.from_numpy(flats[r]).to(DEV)), L._p(slab), parents + 1, ROLE_D[r])
        keep["slab"][r] = slab
        keep["part"][r] = torch.zeros(n * nb[r], dtype=torch.float64, device=DEV)
        keep["dist"][r] = torch.zeros(n + 1, dtype=torch.float32, device=DEV)
        keep["head"][r] = torch.zeros(1, dtype=torch.float32, device=DEV)
        keep["sigma"][r] = torch.full((1,), 0.05, dtype=torch.float32, device=DEV)
    at = lambda r, net: keep["slab"][r].data_ptr() + 4 * net * stride[r]   # noqa: E731
    ref = lambda r: at(r, parents) if with_dist else None                   # noqa: E731
    part = lambda r: L._p(keep["part"][r]) if with_dist else None           # noqa: E731

    def per_role():
        for ri, r in enumerate(ROLES):
            L.call("coevo_fc16_perturb_dist", at(r, 0), L._p(idx), at(r, parents + 1), 0, n, ROLE_D[r], L._p(keep["sigma"][r]),
                   0, 0, ri, flags, None, ref(r), part(r))
            if with_dist:
                L.call("coevo_fc16_distance_finalize", L._p(keep["part"][r]), nb[r], n, L._p(keep["dist"][r]), 1,
                       L._p(keep["head"][r]))

    pj, fj = (L.Perturb16Job * 3)(), (L.FinalizeJob * 3)()
    for ri, r in enumerate(ROLES):
        pj[ri] = L.Perturb16Job(at(r, 0), L._p(idx), at(r, parents + 1), L._p(keep["sigma"][r]), ref(r), part(r), 0, n,
                                ROLE_D[r], 0, ri, 0)
        fj[ri] = L.FinalizeJob(L._p(keep["part"][r]), L._p(keep["dist"][r]), L._p(keep["head"][r]), nb[r], n, 1, 0)

    def multi():
        L.call("coevo_fc16_perturb_dist_multi", ct.cast(pj, ct.c_void_p), 3, 0, flags, None)
        if with_dist:
            L.call("coevo_fc16_distance_finalize_multi", ct.cast(fj, ct.c_void_p), 3)

    k = 2 if with_dist else 1
    return [{"name": f"per-role launches ({3 * k})", "run": per_role, "ms": [], "keep": (keep, idx, pj, fj)},
            {"name": f"multi launches ({k})", "run": multi, "ms": [], "keep": None}]


def event_timed(v, timed):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    v["run"]()
    e1.record()
    e1.synchronize()
    if timed:
        v["ms"].append(e0.elapsed_time(e1))


def host_timed(v, timed):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    v["run"]()
    torch.cuda.synchronize()
    if timed:
        v["ms"].append((time.perf_counter() - t0) * 1e3)


def measure(variants, one, a):
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
    return settle


def table(title, variants, settle, a):
    lines = [f"## {title}", "", f"warm-up {a.warmup}, {settle} settling rounds ({a.settle_ms:.0f} ms), {a.repeats} alternating "
             "timed repeats of each variant.", "", "| variant | median ms | min .. max ms |", "|---|---|---|"]
    for v in variants:
        ms = np.array(v["ms"])
        lines.append(f"| {v['name']} | {np.median(ms):.4f} | {ms.min():.4f} .. {ms.max():.4f} |")
    (a0, a1) = (np.array(v["ms"]) for v in variants)
    disjoint = a0.max() < a1.min() or a1.max() < a0.min()
    lines += ["", f"{variants[1]['name']} median / {variants[0]['name']} median: {np.median(a1) / np.median(a0):.3f}; the ranges "
              + ("are disjoint" if disjoint else "overlap: no speed-up claimed"), ""]
    return lines


def make_args(algorithm, precision, pop, hof, limit, generations):
    import types
    return types.SimpleNamespace(
        algorithm=algorithm, precision=precision, population=pop, hof_size=hof, elites_number=2, generations=generations,
        game="simple_adversary_v3", max_timesteps_per_episode=limit, max_evaluation_steps=limit, adaptive=True,
        mutation_power_agent_0=0.05, mutation_power_agent_1=0.05, mutation_power_adversary=0.05, learning_rate=0.1,
        max_mutation_power=0.2, min_mutation_power=0.001, fitness_sharing=algorithm == "GA", early_stopping=False,
        patience=300, min_delta=0.1, save=False, coevo_rng="device_philox", coevo_seed=0)


def step_variants(algorithm, pop, hof, limit, generations):
    from coevonet_amd.evolutionary_strategy import ESTrainer
    from coevonet_amd.genetic_algorithm import GATrainer
    out = []
    for precision in ("float32", "float16"):
        args = make_args(algorithm, precision, pop, hof, limit, generations)
        env = initialize_env(args)
        torch.manual_seed(1)
        tr = (GATrainer if algorithm == "GA" else ESTrainer)(env, args, collect=False)
        loop = "host-free device loop" if getattr(tr, "device_loop", False) else "host-driven loop"
        out.append({"name": f"{precision} {type(tr).__name__}.step ({loop})", "run": tr.step, "ms": [], "keep": tr})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ga-pop", type=int, default=200)
    ap.add_argument("--hof", type=int, default=5)
    ap.add_argument("--es-pop", type=int, default=1000)
    ap.add_argument("--limit", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=120.0)
    ap.add_argument("--max-generations", type=int, default=4096, help="sizes the float32 device loop's histories")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r19_fp16_trainers.md"))
    a = ap.parse_args()
    assert a.repeats >= 5, "at least 5 repeats of each variant"
    rng = np.random.default_rng(19)
    lines = [f"# float16 trainers: multi breeding launches and whole steps ({torch.cuda.get_device_name(0)})", ""]
    flats = {r: np.stack([random_flat(rng, ROLE_D[r]) for _ in range(3)]) for r in ROLES}
    v = breed_variants(flats, a.ga_pop - 1, 2, True, 0)
    lines += table(f"Co-GA breeding, cfg 2 shape: 3 roles x {a.ga_pop - 1} children from 2 elites, distances fused in (device "
                   "events)", v, measure(v, event_timed, a), a)
    flats = {r: np.stack([random_flat(rng, ROLE_D[r]) for _ in range(2)]) for r in ROLES}
    v = breed_variants(flats, a.es_pop, 1, False, 1)
    lines += table(f"Co-ES perturbation, cfg 3 shape: 3 roles x {a.es_pop} perturbed nets, LayerNorm untouched, no distances "
                   "(device events)", v, measure(v, event_timed, a), a)
    del v
    v = step_variants("GA", a.ga_pop, a.hof, a.limit, a.max_generations)
    lines += table(f"Co-GA step, cfg 2: pop {a.ga_pop}, hof {a.hof}, E 2, T {a.limit}, collect=False (host clock, synchronized)",
                   v, measure(v, host_timed, a), a)
    for x in v:
        x["keep"].finish()
    del v
    v = step_variants("ES", a.es_pop, 1, a.limit, a.max_generations)
    lines += table(f"Co-ES step, cfg 3: pop {a.es_pop}, T {a.limit}, no fitness sharing, collect=False (host clock, synchronized)",
                   v, measure(v, host_timed, a), a)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
