#!/usr/bin/env python3
"""Compare two device-only assembly files kernel by kernel.

    hipcc -O3 --offload-arch=gfx950 -std=c++17 --cuda-device-only -S x.hip -o A.s     (at one commit)
    hipcc ...                                                            -o B.s     (at another)
    tools/isa_diff.py A.s B.s [pattern]

For every kernel symbol (optionally only those matching the regular expression `pattern`) one verdict:
    identical           the same instruction stream
    operand-order only  the same instruction sequence; the files differ only in the order of the two source operands
                        of instructions on the list of commutative ALU ops below, or of the two factors of a 64-bit
                        multiply-add (v_mad_i64_i32, v_mad_u64_u32)
    differs             anything else (a kernel present in one file only included), with both instruction counts and
                        the sgpr / vgpr / spill figures of the code object metadata
Comment and directive lines do not count, and local labels are compared by the position they mark, not by name.
Exit status 1 when any kernel differs, else 0.  What a refactor of kernel source has to show: same code, no GPU needed.
"""
import re
import sys

# Two-source ALU ops whose result does not depend on the order of the sources (carry-out forms left out on purpose)
COMMUTATIVE = frozenset(
    ["s_%s_b%d" % (op, w) for op in ("and", "or", "xor", "nand", "nor", "xnor") for w in (32, 64)]
    + ["s_add_u32", "s_add_i32", "s_mul_i32", "s_min_i32", "s_min_u32", "s_max_i32", "s_max_u32"]
    + ["v_%s%s" % (op, enc) for enc in ("_e32", "_e64", "")
       for op in ("and_b32", "or_b32", "xor_b32", "add_u32", "add_f32", "mul_f32", "min_f32", "max_f32", "mul_lo_u32",
                  "mul_hi_u32", "min_u32", "max_u32", "min_i32", "max_i32", "add_f64", "mul_f64")])

# src0 * src1 + addend: the two factors commute, the addend does not take part
MAD64 = frozenset("v_mad_%s%s" % (t, enc) for t in ("i64_i32", "u64_u32") for enc in ("_e64", ""))

META_KEYS = ("sgpr_count", "vgpr_count", "sgpr_spill_count", "vgpr_spill_count")
_LABEL = re.compile(r"^([.\w$]+):$")
_LOCAL_REF = re.compile(r"\.L[\w$]+")


def parse(text):
    """{kernel symbol: {"insns": [str], "meta": {key: int}}} of one assembly file."""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out = {}
    cur = None          # symbol whose body is being read
    raw, labels = [], {}
    for line in text.splitlines():
        line = line.split(";", 1)[0].strip()
        if not line:
            continue
        m = _LABEL.match(line)
        if m:
            name = m[1]
            if name in kernels:
                cur, raw, labels = name, [], {}
            elif cur is not None and name.startswith(".Lfunc_end"):
                # local labels by position: a branch to the 7th instruction reads the same whatever the label is called
                out[cur] = {"insns": [_LOCAL_REF.sub(lambda r: "@%s" % labels.get(r[0], r[0]), i) for i in raw], "meta": {}}
                cur = None
            elif cur is not None:
                labels[name] = len(raw)
            continue
        if cur is None or line.startswith("."):      # outside a kernel, or a directive
            continue
        raw.append(" ".join(line.split()))
    # code object metadata (YAML in the .amdgpu_metadata block): read by line, one entry per "  - "
    entry = {}
    for line in text.splitlines():
        s = line.strip()
        if line.startswith("  - ") or s == "...":
            entry = {}
            s = s[2:].strip() if line.startswith("  - ") else s
        m = re.match(r"\.(\w+):\s*(\S+)$", s)
        if not m:
            continue
        entry[m[1]] = m[2]
        if "name" in entry and entry["name"] in out:
            out[entry["name"]]["meta"] = {k: int(entry[k]) for k in META_KEYS if k in entry}
    return out


def _operands(insn):
    parts = insn.split(None, 1)
    return parts[0], ([o.strip() for o in parts[1].split(",")] if len(parts) > 1 else [])


def _swapped(x, y):
    """Instructions x, y: the same commutative op on the same destination with its two sources exchanged?"""
    (mx, ox), (my, oy) = _operands(x), _operands(y)
    if mx != my or len(ox) != len(oy):
        return False
    if mx in MAD64:     # dst pair, carry-out, src0, src1, addend: only the two factors may change places
        return len(ox) == 5 and ox[:2] == oy[:2] and ox[4] == oy[4] and ox[2:4] == oy[3:1:-1]
    return mx in COMMUTATIVE and len(ox) == 3 and ox[0] == oy[0] and ox[1:] == oy[:0:-1]


def verdict(a, b):
    """a, b: entries of parse() (or None when the kernel is missing) -> (verdict, detail)."""
    if a is not None and b is not None:
        ia, ib = a["insns"], b["insns"]
        if ia == ib:
            return "identical", ""
        if len(ia) == len(ib):
            diff = [(x, y) for x, y in zip(ia, ib) if x != y]
            if all(_swapped(x, y) for x, y in diff):
                return "operand-order only", "%d of %d instructions" % (len(diff), len(ia))

    def figures(k):
        if k is None:
            return "absent"
        return "%d instructions, %s" % (len(k["insns"]), ", ".join("%s %s" % (key[:-6], k["meta"].get(key, "?")) for key in META_KEYS))
    return "differs", "A: %s | B: %s" % (figures(a), figures(b))


def compare(text_a, text_b, pattern=None):
    """[(symbol, verdict, detail)] over the kernels of both files, in the first file's order."""
    A, B = parse(text_a), parse(text_b)
    names = list(A) + [n for n in B if n not in A]
    if pattern:
        names = [n for n in names if re.search(pattern, n)]
    return [(n,) + verdict(A.get(n), B.get(n)) for n in names]


def main(argv):
    if len(argv) not in (2, 3):
        print(__doc__, file=sys.stderr)
        return 2
    with open(argv[0]) as fa, open(argv[1]) as fb:
        rows = compare(fa.read(), fb.read(), argv[2] if len(argv) == 3 else None)
    counts = {}
    for name, v, detail in rows:
        counts[v] = counts.get(v, 0) + 1
        print("%-18s  %s%s" % (v, name, "  [" + detail + "]" if detail else ""))
    print("%d kernels: %s" % (len(rows), ", ".join("%d %s" % (n, v) for v, n in sorted(counts.items())) or "none"))
    return 1 if counts.get("differs") else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
