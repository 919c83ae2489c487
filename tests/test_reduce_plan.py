"""The plan of the slab reduction (nnf_plan_reduce_set, nn_fac_amd/csrc/k_stream_plan.h) on the CPU: tools/nnf_plan.cpp, a plain
host program over the library's own header, prints the "[nnf reduce]" line of a set; reduce_restatement.plan() states the rule.
The two agree on every case of test_gpu_reduce.CASES and on a sweep around every threshold of the rule, the table reaches what
it has to reach, and reduce_restatement.summed() -- the order of the sums the device is held to -- is checked against math.fsum
where the data makes every order exact."""
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import test_gpu_fused_cross as fused
from reduce_restatement import FORMS, PARTS, cdiv, plan, summed
from test_gpu_reduce import CASES, exact_data, order_data, bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GIB = 1 << 30
# a shape just below and one on each threshold of rows * cols
PRODUCTS = {16: ((255, 257), (256, 256)), 17: ((362, 362), (256, 512)), 18: ((511, 513), (512, 512)),
            19: ((724, 724), (512, 1024)), 21: ((1023, 2050), (1024, 2048))}
SLABS = (1, 2, 3, 4, 7, 8, 15, 16, 17)


@pytest.fixture(scope="module")
def plan_tool():
    tmp = tempfile.mkdtemp(prefix="nnf_plan_reduce_")
    exe = os.path.join(tmp, "nnf_plan")
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-I", os.path.join(ROOT, "nn_fac_amd", "csrc"),
                    os.path.join(ROOT, "tools", "nnf_plan.cpp"), "-o", exe], check=True)
    return exe


def ask(tool, lines):
    p = subprocess.run([tool], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True)
    out = p.stdout.splitlines()
    assert len(out) == len(lines), p.stdout[-2000:]
    return [dict(kv.split("=", 1) for kv in re.findall(r"\S+=\S+", l)) for l in out]


def reduce_line(rows, cols, nslab, lds, stride, align, out64):
    return "reduce rows=%d cols=%d nslab=%d lds=%d stride=%d align=%d out64=%d" % (rows, cols, nslab, lds, stride, align, int(out64))


def test_table_takes_the_forms_it_names(plan_tool):
    cases = list(CASES.values())
    got = ask(plan_tool, [reduce_line(c.rows, c.cols, c.nslab, c.lds, c.stride, c.align, c.out64) for c in cases])
    for c, kv in zip(cases, got):
        assert kv["form"] == c.form, (c.name, kv)
        assert (kv["form"], int(kv["blocks"])) == plan(c.rows, c.cols, c.nslab, c.lds, c.stride, c.align, c.out64), (c.name, kv)
        assert (kv["set"], kv["block0"], int(kv["out64"])) == ("0/1", "0", int(c.out64))


def sweep():
    """(rows, cols, nslab, lds, stride, align, out64) within +-1 of every threshold of rows * cols, at the slab counts around
    every threshold of the slab count, with the conditions of vec4 all met and each failing alone."""
    shapes = [s for pair in PRODUCTS.values() for s in pair] + [(1, 2 ** e + d) for e in PRODUCTS for d in (-1, 0, 1)]
    for rows, cols in shapes:
        lds = cols + (-cols) % 4
        for nslab in SLABS:
            yield rows, cols, nslab, lds, rows * lds, 0, False
            yield rows, cols, nslab, lds, rows * lds, 0, True
            yield rows, cols, nslab, lds + 1, 4 * rows * (lds + 1), 0, False
            yield rows, cols, nslab, lds, rows * lds + 1, 0, False
            for align in (1, 2, 3):
                yield rows, cols, nslab, lds, rows * lds, align, False


def test_plan_around_every_threshold(plan_tool):
    """The library's plan equals the restated rule on the sweep; every form and both answers at every threshold come up."""
    args = list(sweep())
    got = ask(plan_tool, [reduce_line(*a) for a in args])
    seen = set()
    for a, kv in zip(args, got):
        assert (kv["form"], int(kv["blocks"])) == plan(*a), (a, kv)
        seen.add((a[0] * a[1], a[2], kv["form"]))
    assert {f for _, _, f in seen} == set(FORMS)
    for l in (1, 2, 3, 4):           # rows * cols < 2^(20 - l) and nslab >= 2^l: both sides of both
        T, below = 2 ** (20 - l), "par%d" % 2 ** (l - 1) if l > 1 else "plain"
        assert (T - 1, 2 ** l, "par%d" % 2 ** l) in seen and (T, 2 ** l, below) in seen and (T + 1, 2 ** l, below) in seen
        assert (T - 1, 2 ** l - 1, below) in seen
    assert (2 ** 21 - 1, 3, "plain") in seen and (2 ** 21, 3, "vec4") in seen and (2 ** 21 + 1, 3, "vec4") in seen


def test_parts_cap_cannot_bind(plan_tool):
    """A property of the rule, not a case: a parts form has rows * cols < 2^(20 - lg) elements at 256 / 2^lg per workgroup, at
    most 4096 workgroups -- the 4096 cap of those forms never cuts a grid, and a workgroup walks its element loop once.  No
    case can reach the second trip of that loop, and none pretends to."""
    for lg in (1, 2, 3, 4):
        assert cdiv(2 ** (20 - lg) - 1, 256 >> lg) == 4096
    args = [a for a in sweep() if plan(*a)[0] in PARTS]
    for a, kv in zip(args, ask(plan_tool, [reduce_line(*a) for a in args])):
        assert int(kv["blocks"]) == cdiv(a[0] * a[1], 256 // PARTS[kv["form"]]) <= 4096, (a, kv)
    # the caps of the other two forms do bind (test_table_reaches_what_it_names), and the tool's refusals are the entry's
    assert ask(plan_tool, ["reduce rows=0 cols=1 nslab=1", "reduce rows=2 cols=5 nslab=1 lds=4", "reduce rows=2 cols=5 nslab=1 lds=8 stride=12",
                           "reduce rows=2 cols=5 nslab=0"]) == [{"status": "-1"}] * 4


def test_table_reaches_what_it_names():
    cases = list(CASES.values())
    of = lambda form: [c for c in cases if c.form == form]
    total = lambda c: c.rows * c.cols
    assert {c.form for c in cases} == set(FORMS)
    # both sides of every threshold of rows * cols, within 1/64 of it, at a slab count that lets the larger form run
    for l in (1, 2, 3, 4):
        T, P = 2 ** (20 - l), 2 ** l
        below = "par%d" % (P // 2) if l > 1 else "plain"
        assert any(T - T // 64 <= total(c) < T and c.nslab >= P for c in of("par%d" % P)), T
        assert any(T <= total(c) < T + T // 64 and c.nslab >= P for c in of(below)), T
        # and both sides of the slab count
        assert any(c.nslab == P and total(c) < T for c in of("par%d" % P)) and any(c.nslab == P - 1 and total(c) < T for c in of(below)), P
        # lowest and highest slab count of the form below its threshold, and a ragged last workgroup
        if l < 4:
            assert {P, 2 * P - 1} <= {c.nslab for c in of("par%d" % P) if total(c) < T // 2}, P
        assert any(total(c) % (256 // P) for c in of("par%d" % P)), P
    vec_ok = lambda c: not c.out64 and c.lds % 4 == 0 and c.stride % 4 == 0 and c.align == 0
    assert any(2 ** 21 - 2 ** 15 <= total(c) < 2 ** 21 and vec_ok(c) and c.nslab > 1 for c in of("plain"))
    assert any(total(c) == 2 ** 21 for c in of("vec4"))
    # each condition of vec4 failing alone from 2^21 on
    big_plain = [c for c in of("plain") if total(c) >= 2 ** 21]
    fails = lambda c: (c.out64, c.lds % 4 != 0, c.stride % 4 != 0, c.align != 0)
    for k in range(4):
        assert any(fails(c) == tuple(j == k for j in range(4)) for c in big_plain), k
    # parts without a slab, a last part of one
    assert {16, 17, 31, 256, 512} <= {c.nslab for c in of("par16")}
    assert {(1, 1), (50, 50), (255, 257)} <= {(c.rows, c.cols) for c in of("par16")} and any(c.out64 and c.rows == 50 for c in of("par16"))
    # plain: one slab at three sizes; eight-slab batches whole, plus one, two, plus one at both shapes; the 2048-workgroup cap
    assert {(1, 1), (7, 300), (128, 16385)} <= {(c.rows, c.cols) for c in of("plain") if c.nslab == 1}
    for shape in ((512, 1024), (64, 8200)):
        assert {2, 8, 9, 16, 17} <= {c.nslab for c in of("plain") if (c.rows, c.cols) == shape}, shape
    assert any(2048 * 256 < total(c) < 2 * 2048 * 256 for c in of("plain"))          # some threads take a second element, some do not
    # vec4: every column remainder with the last load over NaN padding, the batches of four, the cap
    assert {c.cols % 4 for c in of("vec4")} == {0, 1, 2, 3} and all(c.lds == c.cols + (-c.cols) % 4 for c in of("vec4") if c.cols % 4)
    assert {1, 3, 4, 5, 9} <= {c.nslab for c in of("vec4")}
    assert any(2048 * 256 < c.rows * cdiv(c.cols, 4) < 2 * 2048 * 256 for c in of("vec4")) and any(c.rows * cdiv(c.cols, 4) <= 2048 * 256 for c in of("vec4"))
    assert {(1024, 2048), (128, 16384), (128, 16385), (128, 16386), (128, 16387)} <= {(c.rows, c.cols) for c in of("vec4")}
    # non-finite entries in the last slab of a batch of one, in every form
    assert {c.form for c in cases if c.nonfinite} == set(FORMS)
    assert all(c.nslab % (4 if c.form == "vec4" else 8) == 1 for c in cases if c.nonfinite)
    assert any(c.nonfinite and c.nslab % 8 == 1 for c in of("vec4"))
    # every case has padding columns, NaN between its slabs and stays within 512 slabs
    assert all(c.lds > c.cols and c.stride > c.rows * c.lds and c.nslab <= 512 for c in cases)


@pytest.mark.parametrize("C", [256, 304])
def test_multi_set_pairings(plan_tool, C):
    """The fused cases of test_gpu_fused_cross.py: the slab counts the cross product and the riding Gram take (their own plans,
    through the tool) give the pair of forms the table names -- plain with several slabs, vec4 at remainders 0, 1 and 3, one
    slab, and a plain X H^T tail, each next to the Gram's set."""
    pairs = set()
    for m, n, r, main, gram in fused.BIG_XTY:
        x, g = ask(plan_tool, ["xty %d %d %d %d %d 0 %d" % (C, m, n, r, n, GIB), "gram %d %d %d %d %d 0 %d ldg=%d" % (C, m, m, r, m, GIB, r + 3)])
        ldp = n + (-n) % 4
        assert plan(r, n, int(x["nsplit"]), ldp, r * ldp, 0, False)[0] == main, (m, n, r, x)
        assert g["form"] == "slabs"
        for out64 in (False, True):
            assert plan(r, r, int(g["nsplit"]), r, r * r, 0, out64)[0] == gram, (m, n, r, g)
        pairs.add((main, n % 4 if main == "vec4" else None, int(x["nsplit"]) > 1, gram))
    assert {("plain", None, True, "par2"), ("vec4", 0, True, "par4"), ("vec4", 1, True, "par4"), ("vec4", 3, True, "par2"),
            ("vec4", 1, False, "plain")} == pairs
    for m, n, r, tail, gram in fused.big_xht(C):
        x, g, f = ask(plan_tool, ["xht %d %d %d %d %d 0 %d" % (C, m, n, r, n, GIB), "gram %d %d %d %d %d 0 %d ldg=%d" % (C, n, n, r, n, GIB, r + 3),
                                  "xht_gram %d %d %d %d %d 0 %d ldg=%d" % (C, m, n, r, n, GIB, r + 3)])
        assert int(x["tail_parts"]) >= 4 and f["rides"] == "1", (x, f)
        cols = 16 * int(x["tail_tiles"])
        assert plan(r, cols, int(x["tail_parts"]), cols, r * cols, 0, False)[0] == tail, (m, n, r, x)
        assert plan(r, r, int(g["nsplit"]), r, r * r, 0, False)[0] == gram, (m, n, r, g)
    assert [s[3] for s in fused.big_xht(C)] == ["par4", "plain"]


def small(case):
    return case.nslab * case.rows * case.cols <= 400000 and not case.nonfinite


def test_summed_is_exact_on_the_exact_data():
    """k * 2^-20 entries: every order gives the exactly rounded sum, which is math.fsum's -- in every form."""
    done = set()
    for case in filter(small, CASES.values()):
        slabs, k_sum = exact_data(case, 7)
        want = np.array([math.fsum(col) for col in slabs.reshape(case.nslab, -1).T.astype(np.float64)]).reshape(case.rows, case.cols)
        assert (want * 2.0 ** 20 == k_sum).all()
        for form in FORMS:
            assert (bits(summed(slabs, form)) == bits(want)).all(), (case.name, form)
        done.add(case.form)
    assert done >= {"par16", "par8", "par4", "par2", "plain"}


def test_order_data_tells_the_orders_apart():
    """The second data set is what pins the ORDER: on it the forms differ from each other, a parts form from its own parts added
    in reverse, and a sum that added the last slab twice or left the first out from both."""
    case = CASES["par16_50x50_s17_g64"]
    for span, share in ((15.0, 0.002), (30.0, 0.25)):      # (30 binades of 24-bit entries nearly fit fp64: about 1 sum in 100)
        slabs = order_data(case, 3, span)
        sums = {form: summed(slabs, form) for form in FORMS}
        assert (bits(sums["plain"]) == bits(sums["vec4"])).all()
        for a in ("par2", "par4", "par8", "par16"):
            for b in ("plain", "par2", "par4", "par8", "par16"):
                assert a == b or (bits(sums[a]) != bits(sums[b])).mean() > share, (span, a, b)
        assert (bits(summed(slabs[::-1], "plain")) != bits(sums["plain"])).mean() > share
    # cases with an out64 -- the output that shows the order -- where the order matters: parts of more than one slab
    for form, P in PARTS.items():
        assert any(c.out64 and c.nslab > P + (P == 2) for c in CASES.values() if c.form == form), form
    assert any(c.out64 and c.nslab > 2 for c in CASES.values() if c.form == "plain")


def test_exact_sums_do_round():
    """The fp32 output of the exact data is a real rounding for a good share of the sums: with 512 slabs they are ~2^24 units and
    more, so those with a low bit set do not fit fp32."""
    _, k_sum = exact_data(CASES["par16_50x50_s512"], 0)
    want64 = k_sum.astype(np.float64) * 2.0 ** -20
    assert (want64.astype(np.float32).astype(np.float64) != want64).mean() > 0.05
    assert int(np.abs(k_sum).max()).bit_length() >= 25
