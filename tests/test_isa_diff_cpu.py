"""tools/isa_diff.py on small synthetic assembly texts: one pair per verdict, and the exit status.  No GPU, no compiler."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("isa_diff", os.path.join(ROOT, "tools", "isa_diff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _asm(kernels):
    """A device-only assembly file in the compiler's layout: kernels = [(symbol, function index, body lines, figures)]."""
    text, meta = ["\t.text", "\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\""], ["\t.amdgpu_metadata", "---", "amdhsa.kernels:"]
    for name, idx, body, (sgpr, vgpr, sspill, vspill) in kernels:
        text += ["\t.globl\t%s ; -- Begin function %s" % (name, name), "\t.p2align\t8", "\t.type\t%s,@function" % name,
                 "%s:  ; @%s" % (name, name), "; %bb.0:"]
        text += [ln if ln.endswith(":") else "\t" + ln for ln in body]
        text += ["\ts_endpgm", "\t.section\t.rodata,\"a\",@progbits", "\t.amdhsa_kernel %s" % name,
                 "\t\t.amdhsa_next_free_vgpr %d" % vgpr, "\t.end_amdhsa_kernel", "\t.text", ".Lfunc_end%d:" % idx,
                 "\t.size\t%s, .Lfunc_end%d-%s" % (name, idx, name), "; NumVgprs: %d" % vgpr]
        meta += ["  - .agpr_count:     0", "    .args:", "      - .address_space:  global", "        .offset:         0",
                 "    .name:           %s" % name, "    .sgpr_count:     %d" % sgpr, "    .sgpr_spill_count: %d" % sspill,
                 "    .symbol:         %s.kd" % name, "    .vgpr_count:     %d" % vgpr, "    .vgpr_spill_count: %d" % vspill]
    return "\n".join(text + meta + ["amdhsa.target:   amdgcn-amd-amdhsa--gfx950", "...", "\t.end_amdgpu_metadata", ""])


def _body(idx, and_ops="s[12:13], s[2:3]", extra=()):
    lb = ".LBB%d_2" % idx
    return ["s_load_dwordx2 s[0:1], s[4:5], 0x0  ; a comment", "v_cmp_gt_i32_e32 vcc, s6, v0",
            "s_and_b64 s[8:9], " + and_ops, "s_cbranch_vccz " + lb, "v_add_f32_e32 v1, v2, v3", *extra, lb + ":",
            "v_sub_f32_e32 v4, v1, v2", "global_store_dword v[6:7], v4, off"]


FIG = (20, 34, 0, 0)


def _verdicts(tool, a, b, pattern=None):
    return {name: v for name, v, _ in tool.compare(a, b, pattern)}


def _status(tool, tmp_path, a, b, *pattern):
    pa, pb = tmp_path / "a.s", tmp_path / "b.s"
    pa.write_text(a)
    pb.write_text(b)
    return tool.main([str(pa), str(pb), *pattern])


def test_identical(tmp_path, capsys):
    tool = _tool()
    # the same code behind other label numbers (another function index), other comments and other directives
    a = _asm([("_Z3fooPf", 0, _body(0), FIG), ("_Z3barPf", 1, _body(1), FIG)])
    b = _asm([("_Z3barPf", 4, _body(4), FIG), ("_Z3fooPf", 7, _body(7), FIG)]).replace("; a comment", "; another").replace(
        ".p2align\t8", ".p2align\t9")
    assert _verdicts(tool, a, b) == {"_Z3fooPf": "identical", "_Z3barPf": "identical"}
    assert _status(tool, tmp_path, a, b) == 0
    out = capsys.readouterr().out
    assert out.count("identical") == 3 and "2 kernels: 2 identical" in out


def test_operand_order_only(tmp_path, capsys):
    tool = _tool()
    a = _asm([("_Z3fooPf", 0, _body(0), FIG), ("_Z3barPf", 1, _body(1), FIG)])
    b = _asm([("_Z3fooPf", 0, _body(0, and_ops="s[2:3], s[12:13]"), FIG), ("_Z3barPf", 1, _body(1), FIG)])
    assert _verdicts(tool, a, b) == {"_Z3fooPf": "operand-order only", "_Z3barPf": "identical"}
    assert _status(tool, tmp_path, a, b) == 0
    assert "operand-order only  _Z3fooPf  [1 of 8 instructions]" in capsys.readouterr().out
    # exchanged sources of an op that is NOT commutative are a difference
    c = a.replace("v_sub_f32_e32 v4, v1, v2", "v_sub_f32_e32 v4, v2, v1")
    assert _verdicts(tool, a, c)["_Z3fooPf"] == "differs"
    # ... and so are other sources, or another destination, of one that is
    assert _verdicts(tool, a, a.replace("s[12:13], s[2:3]", "s[2:3], s[14:15]"))["_Z3fooPf"] == "differs"
    assert _verdicts(tool, a, a.replace("s_and_b64 s[8:9], s[12:13], s[2:3]", "s_and_b64 s[10:11], s[2:3], s[12:13]"))["_Z3fooPf"] == "differs"


def test_mad64_factors_commute(tmp_path, capsys):
    tool = _tool()
    mad = "v_mad_u64_u32 v[2:3], s[2:3], v5, s8, v[68:69]"
    a = _asm([("_Z3fooPf", 0, _body(0, extra=(mad,)), FIG)])

    def other(insn):
        return _verdicts(tool, a, _asm([("_Z3fooPf", 0, _body(0, extra=(insn,)), FIG)]))["_Z3fooPf"]
    # the two factors exchanged: destination pair, carry-out and addend as they were
    b = _asm([("_Z3fooPf", 0, _body(0, extra=("v_mad_u64_u32 v[2:3], s[2:3], s8, v5, v[68:69]",)), FIG)])
    assert _verdicts(tool, a, b) == {"_Z3fooPf": "operand-order only"}
    assert _status(tool, tmp_path, a, b) == 0
    assert "operand-order only  _Z3fooPf  [1 of 9 instructions]" in capsys.readouterr().out
    signed = "v_mad_i64_i32 v[2:3], s[2:3], v5, v7, v[68:69]"
    a_signed = _asm([("_Z3fooPf", 0, _body(0, extra=(signed,)), FIG)])
    b_signed = _asm([("_Z3fooPf", 0, _body(0, extra=("v_mad_i64_i32 v[2:3], s[2:3], v7, v5, v[68:69]",)), FIG)])
    assert _verdicts(tool, a_signed, b_signed) == {"_Z3fooPf": "operand-order only"}
    # a swap that involves the addend is another product
    c = _asm([("_Z3fooPf", 0, _body(0, extra=("v_mad_u64_u32 v[2:3], s[2:3], v5, v[68:69], s8",)), FIG)])
    assert _verdicts(tool, a, c) == {"_Z3fooPf": "differs"}
    assert _status(tool, tmp_path, a, c) == 1
    # ... and so are exchanged factors with another addend, carry-out or destination pair, or the other signedness
    assert other("v_mad_u64_u32 v[2:3], s[2:3], s8, v5, v[70:71]") == "differs"
    assert other("v_mad_u64_u32 v[2:3], s[4:5], s8, v5, v[68:69]") == "differs"
    assert other("v_mad_u64_u32 v[4:5], s[2:3], s8, v5, v[68:69]") == "differs"
    assert other("v_mad_i64_i32 v[2:3], s[2:3], s8, v5, v[68:69]") == "differs"


def test_differs(tmp_path, capsys):
    tool = _tool()
    a = _asm([("_Z3fooPf", 0, _body(0), FIG), ("_Z3barPf", 1, _body(1), FIG)])
    b = _asm([("_Z3fooPf", 0, _body(0, extra=("v_mov_b32_e32 v9, 0",)), (24, 36, 2, 1)),
              ("_Z3barPf", 1, _body(1), FIG), ("_Z3newPf", 2, _body(2), FIG)])
    assert _verdicts(tool, a, b) == {"_Z3fooPf": "differs", "_Z3barPf": "identical", "_Z3newPf": "differs"}
    assert _status(tool, tmp_path, a, b) == 1
    out = capsys.readouterr().out
    assert ("differs             _Z3fooPf  [A: 8 instructions, sgpr 20, vgpr 34, sgpr_spill 0, vgpr_spill 0 | "
            "B: 9 instructions, sgpr 24, vgpr 36, sgpr_spill 2, vgpr_spill 1]") in out
    assert "_Z3newPf  [A: absent | B: 8 instructions" in out and "3 kernels: 2 differs, 1 identical" in out
    # a branch that goes somewhere else is a difference although every line reads the same but for the label's place
    moved = _body(0)
    moved.insert(4, moved.pop(5))      # the label one instruction earlier
    assert _verdicts(tool, a, _asm([("_Z3fooPf", 0, moved, FIG), ("_Z3barPf", 1, _body(1), FIG)]))["_Z3fooPf"] == "differs"
    # the pattern restricts the comparison, and with it the exit status
    assert _verdicts(tool, a, b, "bar") == {"_Z3barPf": "identical"}
    assert _status(tool, tmp_path, a, b, "bar") == 0
    assert _status(tool, tmp_path, a, b, "foo|bar") == 1
