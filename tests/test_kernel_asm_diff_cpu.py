"""tools/kernel_asm_diff.py on a small made-up assembly text: what its normalising pass drops, what its label mask hides and
what the per-kernel comparison still sees.  No compiler and no GPU: the tool's own functions on strings."""
import importlib.util
import os

_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "kernel_asm_diff.py")
_spec = importlib.util.spec_from_file_location("kernel_asm_diff", _PATH)
kad = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kad)


def _unit(path, cuid, first, kernels):
    """a translation unit in hipcc's layout: kernels = [(symbol, [instruction lines], vgprs)], numbered from `first`"""
    out = ['\t.text', '\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"', f'\t.file\t"{path}"']
    for i, (sym, insns, vgprs) in enumerate(kernels, first):
        out += [f"\t.globl\t{sym}", f"\t.type\t{sym},@function", f"{sym}:                       ; @{sym}", "; %bb.0:",
                f'\t.loc\t1 {10 + i} 0                 ; {path}:{10 + i}:0']
        out += [ln.replace("@", str(i)) for ln in insns]
        out += ["\ts_endpgm", '\t.section\t.rodata,"a",@progbits', f"\t.amdhsa_kernel {sym}", "\t\t.amdhsa_group_segment_fixed_size 1024",
                f"\t\t.amdhsa_next_free_vgpr {vgprs}", "\t.end_amdhsa_kernel", "\t.text", f".Lfunc_end{i}:",
                f"\t.size\t{sym}, .Lfunc_end{i}-{sym}", f"; NumVgprs: {vgprs}", ""]
    out += [f"\t.type\t__hip_cuid_{cuid},@object", f"\t.globl\t__hip_cuid_{cuid}", f"__hip_cuid_{cuid}:", "\t.byte\t0",
            '\t.ident\t"clang version 19"', ""]
    return "\n".join(out)


LOOP = ["\tv_mov_b32_e32 v0, 0", ".LBB@_1:                                ; =>This Inner Loop Header: Depth=1",
        "\tv_add_u32_e32 v0, 1, v0", "\ts_cbranch_scc1 .LBB@_1", ".LBB@_2:                 ; in Loop: Header=BB@_1 Depth=1"]
A = ("_Z5alphav", LOOP, 12)
B = ("_Z4betav", ["\tv_mov_b32_e32 v1, 1"] + LOOP, 20)
DEAD = ("_Z4deadv", ["\ts_nop 0"], 4)


def test_normalise_drops_what_a_move_may_change_and_nothing_else():
    lines = kad.normalise(_unit("/somewhere/a.hip", "1234abcd", 0, [A]))
    text = "\n".join(lines)
    for gone in ("; %bb.0", ".file", ".loc", ".ident", "__hip_cuid_", "; NumVgprs"):
        assert gone not in text
    assert all(ln.strip() and ln == ln.rstrip() for ln in lines)
    for kept in ("\tv_add_u32_e32 v0, 1, v0", "\ts_cbranch_scc1 .LBB0_1", "\t.amdhsa_kernel _Z5alphav", "\t\t.amdhsa_next_free_vgpr 12",
                 ".Lfunc_end0:", '\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"'):
        assert kept in lines


def test_mask_labels_hides_the_function_index_only():
    assert kad.mask_labels("\ts_cbranch_scc1 .LBB12_3") == "\ts_cbranch_scc1 .LBB#_3"
    assert kad.mask_labels(".Lfunc_end7:") == ".Lfunc_end#:"
    assert kad.mask_labels("\tv_add_u32_e32 v12, 3, v7") == "\tv_add_u32_e32 v12, 3, v7"
    assert kad.mask_labels(".LBB1_3") != kad.mask_labels(".LBB1_4")


def test_a_moved_source_compares_equal():
    same, rows = kad.compare(_unit("/old/place/a.hip", "1234abcd", 0, [A, B]), _unit("/new/place/a.hip", "99ff0000", 0, [A, B]))
    assert same
    assert rows == [("_Z5alphav", 6, 6, 0, True), ("_Z4betav", 7, 7, 0, True)]


def test_a_kernel_removed_in_front_leaves_the_others_equal_per_kernel():
    same, rows = kad.compare(_unit("a.hip", "1", 0, [DEAD, A, B]), _unit("a.hip", "1", 0, [A, B]))
    assert not same   # the whole text lost a kernel and every later label its number
    assert rows == [("_Z4deadv", 2, None, 2, False), ("_Z5alphav", 6, 6, 0, True), ("_Z4betav", 7, 7, 0, True)]


def test_a_changed_instruction_a_changed_label_and_a_changed_descriptor_are_seen():
    old = _unit("a.hip", "1", 0, [A, B])
    swapped = ("_Z4betav", [B[1][0], B[1][1], B[1][3], B[1][2]] + B[1][4:], 20)   # two instructions in the other order
    same, rows = kad.compare(old, _unit("a.hip", "1", 0, [A, swapped]))
    assert not same and rows[0] == ("_Z5alphav", 6, 6, 0, True) and rows[1][:3] == ("_Z4betav", 7, 7) and rows[1][3] > 0 and rows[1][4]
    retarget = ("_Z5alphav", [ln.replace("scc1 .LBB@_1", "scc1 .LBB@_2") for ln in LOOP], 12)   # same opcode, other block
    same, rows = kad.compare(old, _unit("a.hip", "1", 0, [retarget, B]))
    assert not same and rows[0][3] == 2 and rows[0][4] and rows[1] == ("_Z4betav", 7, 7, 0, True)
    same, rows = kad.compare(old, _unit("a.hip", "1", 0, [("_Z5alphav", LOOP, 13), B]))   # one more register
    assert not same and rows[0] == ("_Z5alphav", 6, 6, 0, False)
