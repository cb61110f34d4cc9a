"""The tiled fc1 block of the fp16 DeepQN slab without a GPU: the permutation, the extension header and its binding, every
host-side refusal of the six entry points of include/coevo_ext.h, the Python switches, and the proof that the order-telling nets
of tests/dqn16_tiled_cases.py can see a kernel that adds its k terms in another order."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from coevonet_amd import lib as L
from tests import dqn16_tiled_cases as tc
from tests.test_abi import declared_symbols
from tests.test_fp16_dqn_breeding_cpu import BAD_PERTURB, _perturb_args

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = L.K["COEVO_ERR_ARG"]
EXT = ("coevo_dqn16_forward_argmax_tiled", "coevo_dqn16_forward_hidden_tiled", "coevo_dqn16_pack_tiled",
       "coevo_dqn16_perturb_dist_tiled", "coevo_dqn16_relayout", "coevo_dqn16_unpack_tiled")
TWINS = {"coevo_dqn16_forward_argmax_tiled": "coevo_dqn16_forward_argmax", "coevo_dqn16_forward_hidden_tiled": "coevo_dqn16_forward_hidden",
         "coevo_dqn16_pack_tiled": "coevo_dqn16_pack", "coevo_dqn16_unpack_tiled": "coevo_dqn16_unpack",
         "coevo_dqn16_perturb_dist_tiled": "coevo_dqn16_perturb_dist"}


# ------------------------------------------------------------------------------------------------------- the permutation
def test_the_permutation_is_a_bijection_and_follows_the_documented_rule():
    src, dst = tc.streamed_to_tiled()
    assert len(dst) == 512 * 3136 and np.array_equal(np.sort(dst), np.arange(512 * 3136))
    assert np.array_equal(np.sort(src), np.arange(512 * 3136))
    # the documented rule, element by element: wft16[ob][S][T][lane][j] = fc1.w[64 ob + 16 T + lane % 16][32 S + 4 j + lane / 16]
    h = np.arange(512 * 3136, dtype=np.int64)
    j, lane, T, S, ob = h & 7, (h >> 3) & 63, (h >> 9) & 3, (h >> 11) % 98, (h >> 11) // 98
    out, k = 64 * ob + 16 * T + lane % 16, 32 * S + 4 * j + lane // 16
    assert np.array_equal(tc.tiled_index(out, k), h)
    # the streamed form the library documents (csrc/dqn16_layout.hip.h): [ob][k / 8][out % 64][k % 8]
    e, l, o, ob = h & 7, (h >> 3) & 63, (h >> 9) % 392, (h >> 9) // 392
    assert np.array_equal(tc.streamed_index(64 * ob + l, 8 * o + e), h)
    # a wave's 16-byte pieces of one (S, T) are 1 KiB contiguous; a (task, ob) wave's run is 98 x 4 KiB
    assert tc.tiled_index(64, 0) - tc.tiled_index(0, 0) == 98 * 4 * 64 * 8 and tc.tiled_index(0, 32) - tc.tiled_index(0, 0) == 2048
    assert L.K_EXT["COEVO_DQN16_FC1_SUPER"] == tc.SUPER


def test_the_layout_header_states_the_same_maps(tmp_path):
    """dqn16_fc1_half_to_flat (both forms) and its inverse, compiled for the host from the header itself, against the numpy
    statement on 4096 halves spread over the block and on its corners"""
    src = tmp_path / "maps.cpp"
    src.write_text('#include <hip/hip_runtime.h>\n#include <cstdio>\n#include "dqn16_layout.hip.h"\n'
                   "int main() {\n"
                   "    for (long long i = 0; i < 4100; ++i) {\n"
                   "        const long long h = i < 4096 ? (i * 392087) % (512LL * 3136) : (i == 4096 ? 0 : 512LL * 3136 - (4100 - i));\n"
                   "        const long long fs = coevo::dqn16_fc1_half_to_flat(h), ft = coevo::dqn16_fc1_half_to_flat(h, 1);\n"
                   '        std::printf("%lld %lld %lld %lld %lld\\n", h, fs, ft, (long long)coevo::dqn16_fc1_flat_to_half(fs / 3136, fs % 3136, 0),\n'
                   "                    (long long)coevo::dqn16_fc1_flat_to_half(ft / 3136, ft % 3136, 1));\n"
                   "    }\n    return 0;\n}\n")
    exe = tmp_path / "maps"
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-x", "hip", "--offload-arch=gfx950", "-I",
                    os.path.join(REPO, "coevonet_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    rows = np.array([[int(x) for x in line.split()] for line in
                     subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()])
    assert rows.shape == (4100, 5)
    h, fs, ft = rows[:, 0], rows[:, 1], rows[:, 2]
    assert np.array_equal(rows[:, 3], h) and np.array_equal(rows[:, 4], h), "the inverse maps"
    assert np.array_equal(tc.streamed_index(fs // 3136, fs % 3136), h)
    assert np.array_equal(tc.tiled_index(ft // 3136, ft % 3136), h)


# ------------------------------------------------------------------------------------------------ header, library, binding
def ext_header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "coevo_ext.h")).read(), flags=re.S)


def test_extension_symbols_are_declared_exported_and_bound():
    text = ext_header_text()
    assert sorted(set(re.findall(r"\b(coevo_[a-z0-9_]+)\s*\(", text))) == sorted(EXT) == L.extension_symbols()
    lib, dll = L.load(), ctypes.CDLL(L.LIB_PATH)
    for name in EXT:
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
        assert hasattr(dll, name), f"{name} is not exported by libcoevo.so"
        res, args = L._EXT_SIGS[name]
        assert res is ctypes.c_int and getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
        if name in TWINS:   # the arguments of the streamed twin
            assert L._EXT_SIGS[name] == L._SIGS[TWINS[name]], name
    assert L._EXT_SIGS["coevo_dqn16_relayout"][1] == [ctypes.c_void_p] * 2 + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    # the pinned ABI is what it was: coevo.h declares none of the new names and lib.py's tables for it hold none
    assert L.exported_symbols() == declared_symbols() and len(L.exported_symbols()) == 132
    assert not set(EXT) & set(L._SIGS) and not set(L.K_EXT) & set(L.K) and len(L.STRUCTS) == 17
    assert lib.coevo_version() == 103


def test_the_extension_header_is_plain_c(tmp_path):
    src = tmp_path / "hdr.c"
    src.write_text('#include "coevo_ext.h"\nint main(void) { return coevo_version() + COEVO_DQN16_FC1_SUPER ? 0 : 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"),
                    "-c", str(src), "-o", str(tmp_path / "hdr.o")], check=True)


def test_the_reader_skips_only_the_include_of_coevo_h():
    consts, structs, sigs = L.parse_header('#include "coevo.h"\n#define COEVO_X 3\nint coevo_f(const coevo_dqn_task *t, void *stream);',
                                           known=L.STRUCTS)
    assert consts == {"COEVO_X": 3} and list(sigs) == ["coevo_f"] and set(structs) == set(L.STRUCTS)
    with pytest.raises(L.CoevoError, match="coevo_dqn_task"):   # without the structs of coevo.h the prototype is not readable
        L.parse_header("int coevo_f(const coevo_dqn_task *t);")
    with pytest.raises(L.CoevoError, match="repeats a name"):
        L._parse_ext_header("int coevo_version(void);")
    from coevonet_amd.build import SOURCES, _headers
    assert "dqn16_tiled.hip" in SOURCES and any(h.endswith("coevo_ext.h") for h in _headers())


# ------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("bad", BAD_PERTURB, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD_PERTURB])
def test_perturb_dist_tiled_refuses_what_its_twin_refuses(bad):
    assert L.load().coevo_dqn16_perturb_dist_tiled(*_perturb_args(**bad)) == ERR_ARG


def test_empty_calls_are_ok():
    lib = L.load()
    assert lib.coevo_dqn16_perturb_dist_tiled(*_perturb_args(n=0)) == 0
    assert lib.coevo_dqn16_perturb_dist_tiled(*_perturb_args(n=0, flags=1, ref=None, partial=None)) == 0
    assert lib.coevo_dqn16_relayout(0x10000, 0x20000, 0, 4, 6, 0, 1, None) == 0


def test_pack_unpack_and_relayout_refuse():
    lib = L.load()
    good = dict(a=0x10000, b=0x20000, n=1, C=4, n_actions=6)
    bad = [dict(a=None), dict(b=None), dict(n=0), dict(n=-1), dict(C=0), dict(C=7), dict(C=4 | L.DQN_FC1_TILED), dict(C=4 | 0x200),
           dict(n_actions=0), dict(n_actions=33)]
    for fn in (lib.coevo_dqn16_pack_tiled, lib.coevo_dqn16_unpack_tiled):
        for b in bad:
            a = dict(good, **b)
            assert fn(a["a"], a["b"], a["n"], a["C"], a["n_actions"], None) == ERR_ARG, b
    good = dict(src=0x10000, dst=0x20000, n=1, C=4, n_actions=6, s=0, d=1)
    for b in (dict(src=None), dict(dst=None), dict(dst=0x10000), dict(src=0x10004), dict(src=0x10008), dict(dst=0x20004), dict(n=-1),
              dict(C=0), dict(C=7), dict(C=4 | L.DQN_FC1_TILED), dict(n_actions=0), dict(n_actions=33), dict(s=2), dict(s=-1),
              dict(d=2), dict(d=0x100), dict(s=1, d=3)):
        a = dict(good, **b)
        assert lib.coevo_dqn16_relayout(a["src"], a["dst"], a["n"], a["C"], a["n_actions"], a["s"], a["d"], None) == ERR_ARG, b


def test_forward_pair_refuses_what_its_twins_refuse():
    lib = L.load()
    good = dict(slab=0x10000, tasks=0x20000, n_tasks=1, max_rows=1, rows=1, C=4, n=6, frames=0x30000, actions=0x40000, logits=0x50000,
                status=0x60000, ws=0x70000)
    bad = [dict(slab=None), dict(tasks=None), dict(frames=None), dict(status=None), dict(ws=None), dict(C=0), dict(C=7), dict(n=0),
           dict(n=33), dict(max_rows=0), dict(max_rows=17), dict(n_tasks=0), dict(rows=0), dict(slab=0x10004), dict(slab=0x10008),
           dict(C=4 | L.DQN_FC1_TILED), dict(C=4 | 0x200), dict(C=4 | (1 << 16))]
    for b in bad + [dict(actions=None)]:
        a = dict(good, **b)
        assert lib.coevo_dqn16_forward_argmax_tiled(a["slab"], a["tasks"], a["n_tasks"], a["max_rows"], a["rows"], a["C"], a["n"],
                                                    a["frames"], a["actions"], a["logits"], a["status"], a["ws"], None) == ERR_ARG, b
    for b in bad:
        a = dict(good, **b)
        assert lib.coevo_dqn16_forward_hidden_tiled(a["slab"], a["tasks"], a["n_tasks"], a["max_rows"], a["rows"], a["C"], a["n"],
                                                    a["frames"], a["status"], a["ws"], None) == ERR_ARG, b


# ------------------------------------------------------------------------------------------------------ Python switches
def test_a_bogus_layout_is_refused_before_the_library_is_loaded(monkeypatch):
    from coevonet_amd.dqn_ga_half import HalfDQNGAEngine

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(L, "load", no_load)
    for bogus in ("bogus", "Tiled", None, 1):
        with pytest.raises(ValueError, match="fc1_layout"):
            HalfDQNGAEngine(3, 2, 2, 4, 6, 4, 3, fc1_layout=bogus)
    with pytest.raises(ValueError, match="one rank"):   # the pinned refusals come first
        HalfDQNGAEngine(3, 2, 2, 4, 6, 4, 3, shard=(1, 2), fc1_layout="bogus")


class _Names:
    """what a HalfSynthRollout asks of the library, answered without a GPU"""

    def __init__(self, real):
        self.real, self.log = real, []

    def __getattr__(self, name):
        if name in ("coevo_dqn16_workspace_bytes", "coevo_dqn_workspace_bytes", "coevo_dqn16_slab_stride"):
            return getattr(self.real, name)
        return lambda *a: self.log.append(name) or 0


@pytest.mark.parametrize("tiled", [False, True])
def test_a_half_rollout_on_the_cpu_picks_its_forward_pair(monkeypatch, tiled):
    from coevonet_amd.dqn_ga_half import HalfSynthRollout
    monkeypatch.delenv("COEVO_DQN16_FUSED_OUT", raising=False)
    fake = _Names(L.load())
    monkeypatch.setattr(L, "load", lambda: fake)
    monkeypatch.setattr(L, "_p", lambda t: None if t is None else t.data_ptr())
    slab = torch.zeros(64, dtype=torch.int32)
    ro = HalfSynthRollout([(0, 2), (1, 2), (0, 2)], [0, 16, 32], [5, 6, 7], 4, 6, slab, 123, 0, "cpu", fc1_tiled=tiled)
    assert ro.fc1_tiled is tiled and ro.Cw == 4
    ro._enqueue_lane(ro.lanes[0], 2, None, 0, False)
    hidden = "coevo_dqn16_forward_hidden_tiled" if tiled else "coevo_dqn16_forward_hidden"
    assert fake.log == ["coevo_synth_step", hidden, "coevo_dqn16_out_synth_step", hidden, "coevo_dqn16_out_synth_step"]
    monkeypatch.setenv("COEVO_DQN16_FUSED_OUT", "0")
    ro, fake.log = HalfSynthRollout([(0, 1)], [0, 16], [5], 4, 6, slab, 123, 0, "cpu", fc1_tiled=tiled), []
    ro._enqueue_lane(ro.lanes[0], 1, None, 0, False)
    assert fake.log == ["coevo_synth_step", "coevo_dqn16_forward_argmax_tiled" if tiled else "coevo_dqn16_forward_argmax",
                        "coevo_synth_step"]


# ------------------------------------------------------------------------- the order-telling nets can see a wrong order
def ulps16(a, b):
    """|a - b| in fp16 ulps of the larger magnitude, element by element"""
    a16, b16 = np.asarray(a, dtype=np.float16), np.asarray(b, dtype=np.float16)
    big = np.where(np.abs(a16) >= np.abs(b16), a16, b16)
    return np.abs(a16.astype(np.float64) - b16.astype(np.float64)) / np.spacing(np.abs(big)).astype(np.float64)


@pytest.mark.parametrize("variant", [0, 1])
def test_a_wrong_k_order_changes_an_output_of_every_tile(variant):
    right = tc.telling_hidden(variant)
    assert np.isfinite(right).all() and (right >= 0).all() and len(np.unique(right)) >= 6
    kp, km = tc.telling_pairs(variant)
    # what the list covers: every kk pair inside one quad, the piece seam, every seam of the ring's rounds, both ends, and
    # all of it in every output block and column tile
    lo, hi = np.minimum(kp, km), np.maximum(kp, km)
    same_quad = (lo >> 2) == (hi >> 2)
    assert {(int(a & 3), int(b & 3)) for a, b in zip(lo[same_quad], hi[same_quad])} == set(tc.KK_PAIRS)
    assert ((hi - lo == 1) & (hi % 32 == 0)).reshape(32, 16).any(axis=1).all(), "a piece seam in every tile"
    rounds = {int(b) // (32 * tc.RING) for a, b in zip(lo, hi) if b - a == 1 and b % (32 * tc.RING) == 0}
    assert rounds == set(range(1, tc.SUPER // tc.RING)), "every seam between two rounds of the ring"
    assert ((lo == 0) & (hi == 3135)).reshape(32, 16).any(axis=1).all()
    for name, order in (("k descending", tc.order_descending()), ("kk pairs swapped", tc.order_kk_swapped()),
                        ("j reversed", tc.order_j_reversed())):
        assert sorted(order) == list(range(3136))
        wrong = tc.fc1_rows(tc.telling_fc1(variant), np.zeros(512, dtype=np.float32), np.ones(3136, dtype=np.float32), order)
        seen = (ulps16(wrong, right) >= 1.0).reshape(32, 16).any(axis=1)   # tile t = 4 ob + T holds outputs 16 t .. 16 t + 15
        assert seen.all(), (name, "no output of tiles", np.flatnonzero(~seen).tolist(), "differs by an fp16 ulp")
