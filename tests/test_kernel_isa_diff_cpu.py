"""tools/kernel_isa_diff.py: the part that decides "same instruction stream" is a
pure function over assembly text, tested here on small hand-written snippets in
the compiler's layout (no compiler needed).  What may differ between two equal
kernels: the numbering of the basic-block labels (.LBB<function>_<block>),
comments, and -- outside the kernels -- the file name and the __hip_cuid_ symbol.
Anything else, an opcode or a register, is a difference.  Among the differences
the tool sets one kind apart, `permuted`: equal resources, equally many lines,
and the same lines once their order and the order of a line's operands do not
count (the cases at the end)."""
import importlib.util
import os

import pytest

TOOL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "kernel_isa_diff.py")


@pytest.fixture(scope="module")
def isa():
    spec = importlib.util.spec_from_file_location("kernel_isa_diff", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def unit(file_name, cuid, func, first_block, note, body=None, vgprs=6, helper_first=False):
    """One translation unit with the kernel `axpy_kernel` as function number
    `func`, its blocks numbered from `first_block`."""
    b = [".LBB%d_%d" % (func, first_block + i) for i in range(2)]
    body = body or [
        "s_load_dwordx4 s[0:3], s[4:5], 0x0",
        "v_cmp_gt_i32_e32 vcc, s6, v0 ; %s" % note,
        "s_and_saveexec_b64 s[8:9], vcc",
        "s_cbranch_execz %s" % b[1],
        "%s: ; %%bb.1" % b[0],
        "global_load_dwordx2 v[2:3], v1, s[0:1]",
        "s_waitcnt vmcnt(0)",
        "v_fma_f64 v[2:3], v[2:3], v[4:5], v[2:3]",
        "global_store_dwordx2 v1, v[2:3], s[2:3]",
        "s_cbranch_scc1 %s" % b[0],
        "%s:" % b[1],
        "s_endpgm",
    ]
    helper = """\t.text
\t.globl\t_ZN8smvs_hip11fill_kernelEPdi
\t.type\t_ZN8smvs_hip11fill_kernelEPdi,@function
_ZN8smvs_hip11fill_kernelEPdi: ; @_ZN8smvs_hip11fill_kernelEPdi
; %bb.0:
\tv_mov_b32_e32 v1, 0
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel _ZN8smvs_hip11fill_kernelEPdi
\t\t.amdhsa_next_free_vgpr 2
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{0}:
\t.size\t_ZN8smvs_hip11fill_kernelEPdi, .Lfunc_end{0}-_ZN8smvs_hip11fill_kernelEPdi
; Kernel info:
; TotalNumSgprs: 8
; NumVgprs: 2
; NumAgprs: 0
; ScratchSize: 0
; LDSByteSize: 0 bytes/workgroup (compile time only)
; Occupancy: 8
""".format(func - 1 if helper_first else func + 1)
    kernel = """\t.text
\t.globl\t_ZN8smvs_hip11axpy_kernelEPdS0_i
\t.p2align\t8
\t.type\t_ZN8smvs_hip11axpy_kernelEPdS0_i,@function
_ZN8smvs_hip11axpy_kernelEPdS0_i: ; @_ZN8smvs_hip11axpy_kernelEPdS0_i
; %bb.0: ; {note}
{body}
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel _ZN8smvs_hip11axpy_kernelEPdS0_i
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {vgprs}
\t\t.amdhsa_next_free_sgpr 10
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{func}:
\t.size\t_ZN8smvs_hip11axpy_kernelEPdS0_i, .Lfunc_end{func}-_ZN8smvs_hip11axpy_kernelEPdS0_i
                                        ; -- End function
\t.section\t.AMDGPU.csdata,"",@progbits
; Kernel info:
; codeLenInByte = 96
; TotalNumSgprs: 16
; NumVgprs: {vgprs}
; NumAgprs: 0
; ScratchSize: 0
; LDSByteSize: 0 bytes/workgroup (compile time only)
; Occupancy: 8
""".format(note=note, func=func, vgprs=vgprs,
           body="\n".join(("" if line.startswith(".LBB") else "\t") + line for line in body))
    parts = [helper, kernel] if helper_first else [kernel, helper]
    return ("\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"\n\t.file\t\"%s\"\n" % file_name
            + "".join(parts)
            + "\t.type\t__hip_cuid_%s,@object\n\t.globl\t__hip_cuid_%s\n__hip_cuid_%s:\n\t.byte\t0\n"
            % (cuid, cuid, cuid))


KERNEL = "_ZN8smvs_hip11axpy_kernelEPdS0_i"


def test_label_numbers_comments_file_name_and_cuid_do_not_count(isa):
    a = isa.kernels_of(unit("topology.hip", "1f2e3d", 0, 0, "in range?"))
    b = isa.kernels_of(unit("topo_cut.hip", "abc987", 7, 3, "a different remark", helper_first=True))
    assert set(a) == set(b) == {KERNEL, "_ZN8smvs_hip11fill_kernelEPdi"}
    assert isa.same_kernel(a[KERNEL], b[KERNEL]) == (True, True)
    assert a[KERNEL][0] == dict(vgpr=6, agpr=0, sgpr=16, lds=0, scratch=0, occ=8)
    # the stream starts at the label, holds the descriptor, and names no block by its number
    stream = a[KERNEL][1]
    assert stream[0] == KERNEL + ":"
    assert ".amdhsa_kernel " + KERNEL in stream and ".end_amdhsa_kernel" in stream
    # (numbered in the order they are first named: the branch target, then the loop head)
    assert "s_cbranch_execz .LBB_0" in stream and ".LBB_1:" in stream and ".LBB_0:" in stream
    assert "s_cbranch_scc1 .LBB_1" in stream
    assert not any(".LBB0" in line or ".LBB7" in line for line in stream + b[KERNEL][1])
    assert not any(";" in line or "fill_kernel" in line for line in stream)


def test_blocks_in_another_order_are_a_difference(isa):
    a = isa.normalise_stream(["s_cbranch_execz .LBB2_1", ".LBB2_0:", "s_nop 0", ".LBB2_1:", "s_endpgm"])
    b = isa.normalise_stream(["s_cbranch_execz .LBB5_4", ".LBB5_3:", "s_nop 0", ".LBB5_4:", "s_endpgm"])
    c = isa.normalise_stream(["s_cbranch_execz .LBB5_3", ".LBB5_3:", "s_nop 0", ".LBB5_4:", "s_endpgm"])
    assert a == b
    assert a != c


@pytest.mark.parametrize("old, new", [
    ("v_fma_f64 v[2:3], v[2:3], v[4:5], v[2:3]", "v_mul_f64 v[2:3], v[2:3], v[4:5]"),      # opcode
    ("v_fma_f64 v[2:3], v[2:3], v[4:5], v[2:3]", "v_fma_f64 v[2:3], v[4:5], v[2:3], v[2:3]"),  # operand order
    ("global_load_dwordx2 v[2:3], v1, s[0:1]", "global_load_dwordx2 v[2:3], v6, s[0:1]"),  # register
    ("s_load_dwordx4 s[0:3], s[4:5], 0x0", "s_load_dwordx4 s[0:3], s[4:5], 0x10"),         # offset
])
def test_one_changed_instruction_is_a_difference(isa, old, new):
    a = isa.kernels_of(unit("a.hip", "11", 0, 0, "x"))
    text = unit("a.hip", "11", 0, 0, "x")
    assert text.count(old) == 1
    b = isa.kernels_of(text.replace(old, new))
    assert isa.same_kernel(a[KERNEL], b[KERNEL]) == (True, False)
    # the other kernel of the unit is untouched
    other = "_ZN8smvs_hip11fill_kernelEPdi"
    assert isa.same_kernel(a[other], b[other]) == (True, True)


def test_resources_are_compared_too(isa):
    a = isa.kernels_of(unit("a.hip", "11", 0, 0, "x"))
    b = isa.kernels_of(unit("a.hip", "11", 0, 0, "x", vgprs=8))
    same_resources, same_stream = isa.same_kernel(a[KERNEL], b[KERNEL])
    assert not same_resources
    assert not same_stream       # (the descriptor is part of the stream)


def test_report_counts_missing_and_different_kernels(isa, monkeypatch, capsys):
    monkeypatch.setattr(isa, "demangle", lambda names: {n: "void smvs_hip::" + n + "(double*)" for n in names})
    parent = isa.collect([("topology", unit("topology.hip", "1", 0, 0, "x"))])
    moved = isa.collect([("topo_cut", unit("topo_cut.hip", "2", 4, 2, "y", helper_first=True))])
    assert isa.report(parent, moved) == 0
    out = capsys.readouterr().out
    assert "kernels: parent 2, branch 2" in out and out.count("| same") == 2 and "topo_cut" in out
    fewer = {k: v for k, v in moved.items() if k == KERNEL}
    assert isa.report(parent, fewer) == 1
    assert "only in the parent" in capsys.readouterr().out


# ---- the third verdict: `permuted` (equal resources, equally many lines, the
# same lines once the order of the lines and of a line's operands does not count)
FMA = "v_fma_f64 v[2:3], v[2:3], v[4:5], v[2:3]"
LOAD = "global_load_dwordx2 v[2:3], v1, s[0:1]"
WAIT = "s_waitcnt vmcnt(0)"


def verdict_after(isa, edit, **kw):
    text = unit("a.hip", "11", 0, 0, "x")
    a = isa.kernels_of(text)
    b = isa.kernels_of(edit(unit("a.hip", "11", 0, 0, "x", **kw)))
    return isa.verdict_of(a[KERNEL], b[KERNEL]), isa.permuted_kernel(a[KERNEL], b[KERNEL])


def test_an_unchanged_kernel_is_same_not_permuted_by_name(isa):
    assert verdict_after(isa, lambda t: t) == ("same", True)


def test_two_operands_swapped_is_permuted(isa):
    swapped = "v_fma_f64 v[2:3], v[4:5], v[2:3], v[2:3]"
    assert verdict_after(isa, lambda t: t.replace(FMA, swapped)) == ("permuted", True)


def test_two_lines_swapped_is_permuted(isa):
    def swap(t):
        assert t.count(LOAD + "\n\t" + WAIT) == 1
        return t.replace(LOAD + "\n\t" + WAIT, WAIT + "\n\t" + LOAD)
    assert verdict_after(isa, swap) == ("permuted", True)


@pytest.mark.parametrize("old, new", [
    (FMA, "v_fma_f64 v[2:3], v[2:3], v[6:7], v[2:3]"),   # one operand changed
    (LOAD, "global_load_dwordx2 v[2:3], v1, s[0:1] offset:8"),   # a modifier added
    (FMA, "v_mul_f64 v[2:3], v[2:3], v[4:5]"),   # another opcode
    (WAIT, WAIT + "\n\ts_nop 0"),                # one line added
    (WAIT + "\n", ""),                           # one line removed
])
def test_a_changed_added_or_removed_line_is_different(isa, old, new):
    def edit(t):
        assert t.count(old) == 1
        return t.replace(old, new)
    assert verdict_after(isa, edit) == ("DIFFERENT", False)


def test_changed_resources_are_not_permuted(isa):
    verdict, permuted = verdict_after(isa, lambda t: t, vgprs=8)
    assert not permuted
    assert verdict == "DIFFERENT (resources differ)"
    # ... even where the stream itself is only reordered
    a = isa.kernels_of(unit("a.hip", "11", 0, 0, "x"))[KERNEL]
    b = (dict(a[0], sgpr=a[0]["sgpr"] + 2), list(reversed(a[1])))
    assert not isa.permuted_kernel(a, b)
    assert isa.permuted_kernel(a, (a[0], list(reversed(a[1]))))


def test_report_counts_permuted_kernels_apart(isa, monkeypatch, capsys):
    monkeypatch.setattr(isa, "demangle", lambda names: {n: "void smvs_hip::" + n + "(double*)" for n in names})
    parent = isa.collect([("a", unit("a.hip", "1", 0, 0, "x"))])
    text = unit("b.hip", "2", 0, 0, "x")
    swapped = isa.collect([("b", text.replace(FMA, "v_fma_f64 v[2:3], v[4:5], v[2:3], v[2:3]"))])
    assert isa.report(parent, swapped) == 0
    out = capsys.readouterr().out
    assert out.count("| permuted") == 1 and out.count("| same") == 1
    assert "0 of 2 kernels differ or are missing on one side, 1 are permuted" in out
    changed = isa.collect([("b", text.replace(FMA, "v_mul_f64 v[2:3], v[2:3], v[4:5]"))])
    assert isa.report(parent, changed) == 1
    assert "| DIFFERENT" in capsys.readouterr().out
