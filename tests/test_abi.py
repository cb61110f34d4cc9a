"""The C ABI in one place (no compute: runs without a GPU): libcoevo.so exports every symbol include/coevo.h declares, the
tables coevonet_amd/lib.py derives from the header equal the hand-written ones they replaced (tests/golden/abi_tables.json),
its struct mirrors have the compiler's layout, the header reader fails loudly, and every float16 feature's entry points are
declared, exported and bound with the signatures they were introduced with."""
import ctypes
import json
import os
import re
import subprocess

import pytest

from coevonet_amd import lib as L
from tests.golden import make_golden_abi as ma

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_text():
    """include/coevo.h without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "coevo.h")).read(), flags=re.S)


def declared_symbols():
    return sorted(set(re.findall(r"\b(coevo_[a-z0-9_]+)\s*\(", header_text())))


def test_library_exports_every_declared_symbol():
    from coevonet_amd.build import build
    build()
    dll = ctypes.CDLL(L.LIB_PATH)
    names = declared_symbols()
    assert len(names) >= 15
    for n in names:
        assert hasattr(dll, n), f"{n} declared in include/coevo.h but not exported"
    assert sorted(L.exported_symbols()) == names, "lib.py binds a different set than the header declares"


def test_version_and_layout_constants():
    dll = L.load()
    assert dll.coevo_version() == 103
    # parameter counts of the reference's FCNetwork (139 781 good / 138 757 adversary)
    assert L.fc_param_count(10) == 139781 and L.fc_param_count(8) == 138757
    assert L.fc_slab_stride(10) % 64 == 0 and L.fc_slab_stride(10) >= 139781
    assert L.fc_param_count(9) < 0  # unsupported width is an argument error, not a crash


def test_graft_entry_build_runs():
    """the driver's "does it build" check (__graft_entry__.build): compiles what is stale, builds the oracle's C restatement,
    binds every symbol and compares the library's version with the header's (a hard-coded number there went stale in round 5)"""
    import importlib
    import sys
    sys.path.insert(0, REPO)
    g = importlib.import_module("__graft_entry__")
    g.build()


def test_header_is_plain_c(tmp_path):
    """include/coevo.h is the drop-in boundary: it must compile as C99 (what a cgo / JNI / ctypes-gen binding includes)"""
    src = tmp_path / "hdr.c"
    src.write_text('#include "coevo.h"\nint main(void) { return coevo_version() ? 0 : 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"),
                    "-c", str(src), "-o", str(tmp_path / "hdr.o")], check=True)


# ------------------------------------------------------------------------------- the derived tables against the fixture
# the argument positions lib.py typed POINTER(...) by hand; derived, they are c_void_p like every other pointer (byref(),
# ctypes arrays and None pass as before)
WAS_TYPED_POINTER = {("coevo_mpe_rollout", 0): "POINTER(RolloutDesc)", ("coevo_mpe16_rollout", 0): "POINTER(RolloutDesc)",
                     ("coevo_mpe_host_rollout", 1): "POINTER(HostRolloutDesc)",
                     ("coevo_dqn_host_frames_rollout", 1): "POINTER(FramesRolloutDesc)",
                     ("coevo_rollout_ctx_light_times", 1): "POINTER(c_float)"}


def test_derived_tables_equal_the_hand_written_ones():
    """every restype, argtype, struct field (name, type, offset, size), sizeof and constant renders as it did when lib.py
    spelled them out, except the five positions above; any sixth difference fails"""
    want = json.load(open(ma.FIXTURE))
    got = json.loads(json.dumps(ma.render(L)))
    assert len(want["sigs"]) == 132 and len(want["structs"]) == 14
    for (name, i), was in WAS_TYPED_POINTER.items():
        assert want["sigs"][name]["argtypes"][i] == was, (name, i)
        assert got["sigs"][name]["argtypes"][i] == "c_void_p", (name, i)
        want["sigs"][name]["argtypes"][i] = "c_void_p"
    for table in ("sigs", "structs", "constants"):
        assert sorted(got[table]) == sorted(want[table]), table
        for key in want[table]:
            assert got[table][key] == want[table][key], (table, key)


def test_struct_mirrors_have_the_compilers_layout(tmp_path):
    """sizeof and every field's offsetof / size of every struct in the header, as gcc lays them out, against ctypes"""
    assert len(L.STRUCTS) == 17
    c_field = lambda struct, f: "pcg_" + f if struct == "coevo_pcg64" else f   # (PCG64State drops the header's prefix)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "coevo.h"', "int main(void) {"]
    want = []
    for name, cls in L.STRUCTS.items():
        lines.append(f'    printf("{name} %zu\\n", sizeof({name}));')
        want.append(f"{name} {ctypes.sizeof(cls)}")
        for f, _ in cls._fields_:
            cf = c_field(name, f)
            lines.append(f'    printf("{name}.{cf} %zu %zu\\n", offsetof({name}, {cf}), sizeof((({name} *)0)->{cf}));')
            want.append(f"{name}.{cf} {getattr(cls, f).offset} {getattr(cls, f).size}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o",
                    str(tmp_path / "layout")], check=True)
    got = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines()
    assert got == want


# --------------------------------------------------------------------------------------------- the reader fails loudly
def test_reader_parses_the_headers_forms():
    text = """
    /* a comment with a ; and a ( in it */
    #ifndef X_H
    #define X_H
    #ifdef __cplusplus
    extern "C" {
    #endif
    #define COEVO_A 3
    #define COEVO_B 0x10   /* hex */
    #define COEVO_NEG (-2)
    #define COEVO_AB (COEVO_A * COEVO_B)
    typedef struct { uint64_t pcg_state_hi, pcg_state_lo; } coevo_pair;
    typedef struct coevo_tagged {
        const coevo_pair *tasks[2];   /* two pointers */
        int32_t game_first, count; uint64_t first_ordinal;
        float *pop, *hof;
        int32_t n_tasks[2];
        coevo_pair rng;
    } coevo_tagged;
    int coevo_version(void);
    const char *coevo_flags(void);
    void coevo_destroy(void *ctx);
    int64_t coevo_split(const float *slab,
                        const coevo_tagged *desc /* host */, coevo_pair rng,
                        size_t bytes, double lr, uint32_t lo,
                        void *stream);
    #ifdef __cplusplus
    }
    #endif
    #endif
    """
    consts, structs, sigs = L.parse_header(text)
    assert consts == {"COEVO_A": 3, "COEVO_B": 16, "COEVO_NEG": -2, "COEVO_AB": 48}
    pair, tagged = structs["coevo_pair"], structs["coevo_tagged"]
    assert list(structs) == ["coevo_pair", "coevo_tagged"]
    assert pair._fields_ == [("pcg_state_hi", ctypes.c_uint64), ("pcg_state_lo", ctypes.c_uint64)]
    assert tagged._fields_ == [("tasks", ctypes.c_void_p * 2), ("game_first", ctypes.c_int32), ("count", ctypes.c_int32),
                               ("first_ordinal", ctypes.c_uint64), ("pop", ctypes.c_void_p), ("hof", ctypes.c_void_p),
                               ("n_tasks", ctypes.c_int32 * 2), ("rng", pair)]
    assert sigs == {"coevo_version": (ctypes.c_int, []), "coevo_flags": (ctypes.c_char_p, []),
                    "coevo_destroy": (None, [ctypes.c_void_p]),
                    "coevo_split": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_void_p, pair, ctypes.c_size_t, ctypes.c_double,
                                                     ctypes.c_uint32, ctypes.c_void_p])}


@pytest.mark.parametrize("text, names", [
    ("int coevo_f(short n, void *stream);", ("short", "coevo_f")),                              # an unknown scalar type
    ("int coevo_g(unsigned int n);", ("unsigned int n", "coevo_g")),
    ("int coevo_h(coevo_nowhere desc, void *stream);", ("coevo_nowhere", "coevo_h")),            # an unknown struct, by value
    ("int coevo_i(const coevo_nowhere *desc);", ("coevo_nowhere", "coevo_i")),                   # ... and behind a pointer
    ("typedef struct { int32_t n; coevo_nowhere d; } coevo_s;", ("coevo_nowhere", "coevo_s")),
    ("typedef struct { int32_t n : 3; } coevo_bits;", ("coevo_bits",)),
    ("int coevo_j(void x);", ("coevo_j",)),
    ("int coevo_k(int (*fn)(int));", ("coevo_k",)),
    ("int coevo_l;", ("coevo_l",)),
    ("#define COEVO_A 1\n#define COEVO_SUM (COEVO_A + 1)", ("COEVO_SUM (COEVO_A + 1)",)),        # outside the #define grammar
    ("#define COEVO_LATER (COEVO_UNSEEN * 2)", ("COEVO_LATER",)),
    ("#define COEVO_SHIFT (1 << 4)", ("COEVO_SHIFT (1 << 4)",)),
    ("#define COEVO_F(x) 3", ("COEVO_F(x) 3",)),
    ("#define COEVO_OCT 010", ("COEVO_OCT 010",)),
])
def test_reader_raises_and_names_the_declaration(text, names):
    with pytest.raises(L.CoevoError) as e:
        L.parse_header(text)
    for n in names:
        assert n in str(e.value), str(e.value)


def test_a_missing_header_is_an_error_that_names_the_path(monkeypatch, tmp_path):
    gone = str(tmp_path / "include" / "coevo.h")
    monkeypatch.setattr(L, "HEADER_PATH", gone)
    with pytest.raises(L.CoevoError, match=re.escape(gone)):
        L._header_text()


# ---------------------------------------------------------------- the float16 features' entry points, one case per feature
# names: declared in the header with this return type, exported by the library, bound by lib.py (int64: the ones that return
# int64_t; the others return int).  same: (entry point, its float32 counterpart, the counterpart's argument positions it
# lacks) - equal restype and argtypes otherwise, slab pointers untyped.  header: what else the comment-stripped header says.
FEATURES = {
    "fp16_rollout": dict(
        names=("coevo_mpe16_policy_cycle", "coevo_mpe16_rollout"),
        same=[("coevo_mpe16_rollout", "coevo_mpe_rollout", ()),   # the rollout takes the existing descriptor
              ("coevo_mpe16_policy_cycle", "coevo_mpe_policy_cycle_fused", ())]),
    "fp16_breeding": dict(
        names=("coevo_fc16_perturb_dist", "coevo_fc16_distance", "coevo_fc16_distance_finalize", "coevo_fc16_gather",
               "coevo_ga16_promote", "coevo_fc16_perturb_blocks"),
        int64=("coevo_fc16_perturb_blocks",),
        same=[("coevo_fc16_perturb_dist", "coevo_fc_perturb_dist", ()),
              ("coevo_fc16_distance_finalize", "coevo_fc_distance_finalize", ()),
              ("coevo_fc16_gather", "coevo_fc_gather", ()), ("coevo_ga16_promote", "coevo_ga_promote", ())],
        header=[r"typedef struct coevo_ga16_promote_role\s*\{\s*void \*pop, \*hof, \*elite;"]),
    "fp16_es": dict(
        names=("coevo_es16_partial_floats", "coevo_es16_fitness", "coevo_es16_partial", "coevo_es16_apply"),
        int64=("coevo_es16_partial_floats",)),
    "fp16_trainers": dict(
        names=("coevo_fc16_perturb_dist_multi", "coevo_fc16_distance_finalize_multi"),
        same=[("coevo_fc16_perturb_dist_multi", "coevo_fc_perturb_dist_multi", ()),
              ("coevo_fc16_distance_finalize_multi", "coevo_fc_distance_finalize_multi", ())],
        header=[r"\}\s*coevo_fc16_perturb_job\s*;"]),
    "fp16_dqn": dict(
        names=("coevo_dqn16_slab_stride", "coevo_dqn16_pack", "coevo_dqn16_unpack", "coevo_dqn16_workspace_bytes",
               "coevo_dqn16_forward_argmax"),
        int64=("coevo_dqn16_slab_stride", "coevo_dqn16_workspace_bytes")),
    "fp16_dqn_breeding": dict(
        names=("coevo_dqn16_perturb_dist", "coevo_dqn16_distance", "coevo_dqn16_perturb_blocks"),
        int64=("coevo_dqn16_perturb_blocks",),
        same=[("coevo_dqn16_perturb_dist", "coevo_dqn_perturb", (12,))]),   # coevo_dqn_perturb's argument list without E
    "fp16_dqn_es": dict(
        names=("coevo_dqn_es16_partial_floats", "coevo_dqn_es16_partial", "coevo_dqn_es16_apply"),
        int64=("coevo_dqn_es16_partial_floats",)),
    "fp16_dqn_trainers": dict(
        names=("coevo_dqn16_forward_hidden", "coevo_dqn16_out_synth_step"),
        same=[("coevo_dqn16_out_synth_step", "coevo_dqn_out_synth_step", ()),
              # coevo_dqn16_forward_argmax's arguments without actions and logits
              ("coevo_dqn16_forward_hidden", "coevo_dqn16_forward_argmax", (8, 9))]),
}


@pytest.mark.parametrize("feature", sorted(FEATURES))
def test_feature_entry_points_are_declared_exported_and_bound(feature):
    f = FEATURES[feature]
    text = header_text()
    lib = L.load()
    dll = ctypes.CDLL(L.LIB_PATH)
    for name in f["names"]:
        ret, res = ("int64_t", ctypes.c_int64) if name in f.get("int64", ()) else ("int", ctypes.c_int)
        assert re.search(rf"\b{ret}\s+{name}\s*\(", text), f"{name} is not declared in include/coevo.h as returning {ret}"
        assert name in declared_symbols()
        assert hasattr(dll, name), f"{name} is not exported by libcoevo.so"
        assert name in L.exported_symbols(), f"{name} is not bound in lib.py"
        assert L._SIGS[name][0] is res
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == L._SIGS[name][1], name
    for name, other, lacks in f.get("same", ()):
        want = [a for i, a in enumerate(L._SIGS[other][1]) if i not in lacks]
        assert len(want) == len(L._SIGS[other][1]) - len(lacks)
        assert L._SIGS[name] == (L._SIGS[other][0], want), (name, other)
    for pattern in f.get("header", ()):
        assert re.search(pattern, text), pattern
    assert re.search(r"#define COEVO_VERSION 103\b", text) and lib.coevo_version() == 103


def test_fp16_perturb_job_has_the_fp32_jobs_layout():
    """coevo_fc16_perturb_job: the field order of coevo_fc_perturb_job over untyped slabs, 72 bytes, as the kernels' source
    asserts"""
    assert ctypes.sizeof(L.Perturb16Job) == 72 == ctypes.sizeof(L.PerturbJob)
    assert [f[0] for f in L.Perturb16Job._fields_] == [f[0] for f in L.PerturbJob._fields_]
    for name, _ in L.PerturbJob._fields_:
        assert getattr(L.Perturb16Job, name).offset == getattr(L.PerturbJob, name).offset, name
        assert getattr(L.Perturb16Job, name).size == getattr(L.PerturbJob, name).size, name
    src = open(os.path.join(REPO, "coevonet_amd", "csrc", "fc16_offspring.hip")).read()
    assert re.search(r"static_assert\(sizeof\(coevo_fc16_perturb_job\) == 72", src)
