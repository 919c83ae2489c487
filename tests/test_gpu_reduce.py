"""Every form of the fixed-order slab reduction (nn_fac_amd/csrc/k_reduce.hip) bit for bit, through nnf_reduce_slabs_f32 on
slabs this file lays out, and nnf_sum_f64, the one-workgroup tail of the cost kernels.  The reduction is what every split launch
of the library ends in (W^T X, the X H^T tail, the Gram, the right MU update, MTTKRP, the dimension tree); it promises fp64 sums
in a fixed order and one rounding to fp32, which is more than the 1e-5 of its callers' tests can see.

CASES names every case with the form it must take (test_reduce_plan.py holds the table against the plan on the CPU and checks
what it reaches; here the form is read from the library's own NNF_REDUCE_DEBUG line, in one child process).  All comparisons
are equality of BITS, on two sets of data:
  exact -- entries k * 2^-20, |k| < 2^20 random integers: every partial sum of up to 512 slabs in any order has at most 30
           significant bits and is exact in fp64, so the reference is integer arithmetic (int64) and does not depend on the order
           of the sums, nor on the code under test; out64 is that sum, out its rounding to fp32;
  order -- +-2^U(-15, 15) * U(1, 2): the order of the additions changes the fp64 sum, which must be
           reduce_restatement.summed(slabs, form).  (It is out64 that sees the order -- the fp32 rounding hides the last bits
           of an fp64 sum -- so every form that can have an out64 has cases with one at slab counts where the orders differ;
           those cases run a second set over 60 binades as well, on which most sums depend on the order.)
The slabs lie in a pool of NaN: the padding columns of a slab row (lds > cols) and the floats between two slabs stay NaN; out
is a block inside a buffer of NaN sentinels with ldo > cols and a guard row on both sides."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from reduce_restatement import plan, summed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NNF_ERR_ARG = -1
SENTINEL32, SENTINEL64 = 0x7FC00ABC, 0x7FF8000000000ABC      # NaNs with a payload nothing computes
LDO_PAD, GAP = 3, 8

Case = collections.namedtuple("Case", "name rows cols nslab lds stride align out64 form nonfinite")


def _case(rows, cols, nslab, form, lds=None, gap=GAP, align=0, out64=False, nonfinite=False, tag=""):
    """lds: by default the next multiple of 4 above cols (cols + 4 where cols is one), so that every row has NaN padding and a
    16-byte load of the last quad of a row covers it; gap: NaN floats between two slabs."""
    if lds is None:
        lds = cols + 4 - cols % 4
    name = "%s_%dx%d_s%d%s%s%s" % (form, rows, cols, nslab, "_g64" if out64 else "", "_nonfinite" if nonfinite else "", tag)
    return Case(name, rows, cols, nslab, lds, rows * lds + gap, align, out64, form, nonfinite)


def reduce_cases():
    c = [
        # ---- par16: rows * cols < 2^16, 16 slabs and more; 17 and 31 slabs leave parts without a slab and a last part of one
        _case(1, 1, 16, "par16"), _case(1, 1, 512, "par16"), _case(1, 1, 31, "par16", out64=True),
        _case(50, 50, 16, "par16", out64=True), _case(50, 50, 17, "par16", out64=True), _case(50, 50, 256, "par16", out64=True),
        _case(50, 50, 512, "par16"), _case(255, 257, 16, "par16"), _case(255, 257, 31, "par16"),
        _case(255, 257, 17, "par16", out64=True, nonfinite=True),
        # ---- par8: 8 .. 15 slabs below 2^16, any count from 8 in [2^16, 2^17)
        _case(30, 700, 8, "par8"), _case(30, 700, 15, "par8", out64=True), _case(256, 256, 8, "par8"), _case(256, 256, 15, "par8"),
        _case(256, 256, 17, "par8"), _case(362, 362, 8, "par8"), _case(362, 362, 33, "par8"),
        _case(30, 700, 9, "par8", nonfinite=True),
        # ---- par4: 4 .. 7 slabs below 2^17, any count from 4 in [2^17, 2^18)
        _case(30, 700, 4, "par4"), _case(362, 362, 7, "par4"), _case(256, 512, 4, "par4"), _case(256, 512, 8, "par4"),
        _case(511, 513, 4, "par4", out64=True), _case(511, 513, 7, "par4", out64=True), _case(511, 513, 17, "par4"),
        _case(256, 512, 9, "par4", nonfinite=True),
        # ---- par2: 2 or 3 slabs below 2^18, any count from 2 in [2^18, 2^19)
        _case(7, 300, 2, "par2"), _case(511, 513, 3, "par2"), _case(512, 512, 2, "par2"), _case(512, 512, 4, "par2"),
        _case(724, 724, 2, "par2", out64=True), _case(724, 724, 3, "par2"), _case(724, 724, 16, "par2", out64=True),
        _case(512, 512, 9, "par2", nonfinite=True),
        # ---- plain: one slab at any size below 2^21; from 2^19 on with slabs in whole batches of eight, plus one, two, plus one
        _case(1, 1, 1, "plain"), _case(7, 300, 1, "plain", out64=True), _case(724, 724, 1, "plain"),
        _case(128, 16385, 1, "plain", out64=True),
        *[_case(512, 1024, s, "plain") for s in (2, 8, 9, 16, 17)],
        # (64 x 8200 = 524800 elements: more than 2048 workgroups of 256, so 512 threads take a second element)
        *[_case(64, 8200, s, "plain", out64=s == 8) for s in (2, 8, 16, 17)],
        _case(64, 8200, 9, "plain", out64=True, nonfinite=True),
        # below 2^21 with everything else in place for vec4
        _case(1023, 2050, 3, "plain"),
        # from 2^21 on, each of the four conditions of vec4 failing alone
        _case(1024, 2048, 3, "plain", out64=True), _case(1024, 2048, 3, "plain", lds=2053, tag="_lds1"),
        _case(1024, 2048, 3, "plain", gap=GAP + 1, tag="_stride1"), _case(1024, 2048, 3, "plain", align=1, tag="_align1"),
        # ---- vec4: from 2^21 on; column remainders 1, 2, 3 with lds the next multiple of 4: the last load of a row covers NaN
        # padding.  128 x 16385 is the smallest shape of the table with more than 2048 x 256 quads (524416)
        _case(1024, 2048, 1, "vec4"), _case(1024, 2048, 4, "vec4"), _case(128, 16384, 3, "vec4"), _case(128, 16385, 9, "vec4"),
        _case(128, 16386, 4, "vec4"), _case(128, 16387, 5, "vec4"), _case(128, 16385, 1, "vec4"),
        _case(128, 16387, 5, "vec4", nonfinite=True), _case(128, 16385, 9, "vec4", nonfinite=True),
    ]
    out = collections.OrderedDict((k.name, k) for k in c)
    assert len(out) == len(c)
    return out


CASES = reduce_cases()
POOL_FLOATS = max(k.nslab * k.stride + k.align for k in CASES.values()) + 64
assert POOL_FLOATS * 4 < 80 << 20            # the largest set: 9 slabs of 128 x 16388 floats


# ---- the data and its references (NumPy, CPU) ----
def exact_data(case, seed):
    """(slabs as float32, the exact sums as int64 in units of 2^-20)."""
    rng = np.random.default_rng(seed)
    k = rng.integers(-(2 ** 20) + 1, 2 ** 20, size=(case.nslab, case.rows, case.cols), dtype=np.int32)
    assert case.nslab <= 512 and case.nslab * 2 ** 20 < 2 ** 53      # every partial sum is an integer fp64 holds exactly
    return (k.astype(np.float32) * np.float32(2.0 ** -20)), k.sum(axis=0, dtype=np.int64)


def order_data(case, seed, span=15.0):
    """+-2^U(-span, span) * U(1, 2).  Over 30 binades the 24-bit entries span 54 bits, one more than fp64 holds: the order shows
    in about one sum of a hundred (test_reduce_plan.py counts them).  span = 30 is a second set on which most sums show it."""
    rng = np.random.default_rng(seed)
    shape = (case.nslab, case.rows, case.cols)
    mag = np.exp2(2.0 * span * rng.random(size=shape, dtype=np.float32) - span) * (1.0 + rng.random(size=shape, dtype=np.float32))
    return np.where(rng.random(size=shape, dtype=np.float32) < 0.5, -mag, mag).astype(np.float32)


def nonfinite_spots(case):
    """(row, col, slab values by slab index, expected) of the four poisoned outputs: a NaN, a +Inf and a -Inf each in one entry
    of the LAST slab -- the slab whose clamped duplicate loads fill the batch (nslab % 8 == 1, % 4 == 1 for vec4) -- and one
    element with +Inf in slab 0 and -Inf in the last."""
    r, c, last = case.rows, case.cols, case.nslab - 1
    assert case.nslab % (4 if case.form == "vec4" else 8) == 1
    spots = [(r - 1, c - 1, {last: np.nan}, np.nan), (0, 0, {last: np.inf}, np.inf), (r // 2, c // 3, {last: -np.inf}, -np.inf),
             (r // 3, c - 2, {0: np.inf, last: -np.inf}, np.nan)]
    assert len({(a, b) for a, b, _, _ in spots}) == 4
    return spots


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


# ---- the device side ----
@pytest.fixture(scope="module")
def eng(built_lib):
    from nn_fac_amd.engine import get_engine
    return get_engine("cuda:0")


@pytest.fixture(scope="module")
def pool(built_lib):
    return torch.empty(POOL_FLOATS + 4, device="cuda")


def aligned(pool):
    """The pool from its first 16-byte boundary on (the allocator's blocks start on one; this does not rely on it)."""
    return pool[(-(pool.data_ptr() // 4)) % 4:]


def lay_out(case, slabs, pool):
    """NaN everywhere, the slabs at `align` floats past a 16-byte boundary; returns (device view of the set, its host image)."""
    img = np.full(case.nslab * case.stride, np.nan, dtype=np.float32)
    np.lib.stride_tricks.as_strided(img, (case.nslab, case.rows, case.cols), (4 * case.stride, 4 * case.lds, 4))[...] = slabs
    pool.fill_(float("nan"))
    dev = aligned(pool)[case.align:case.align + img.size]
    assert dev.data_ptr() % 16 == 4 * case.align
    dev.copy_(torch.from_numpy(img))
    return dev, img


def sentinels(shape, dtype):
    if dtype == torch.float32:
        return torch.full(shape, SENTINEL32, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full(shape, SENTINEL64, dtype=torch.int64, device="cuda").view(torch.float64)


def call_reduce(eng, case, dev, status=0, guards=True):
    """One call on the set `dev`; returns (out, out64 or None) as NumPy after checking every sentinel around them (guards)."""
    from nn_fac_amd import _lib
    ldo = case.cols + LDO_PAD
    buf = sentinels((case.rows + 2, ldo), torch.float32)
    buf64 = sentinels((case.rows * case.cols + 16,), torch.float64) if case.out64 else None
    rc = eng.lib.nnf_reduce_slabs_f32(eng.ctx, dev.data_ptr(), case.nslab, case.stride, case.rows, case.cols, case.lds,
                                      buf[1].data_ptr(), ldo, buf64[8:].data_ptr() if case.out64 else None, eng._stream())
    assert rc == status, _lib.load().nnf_status_string(rc)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    guard = np.ones(got.shape, dtype=bool)
    guard[1:case.rows + 1, :case.cols] = False
    assert not guards or (bits(got)[guard] == SENTINEL32).all(), "%s: a sentinel around out was overwritten" % case.name
    got64 = None
    if case.out64:
        b64 = buf64.cpu().numpy()
        assert not guards or ((bits(b64[:8]) == SENTINEL64).all() and (bits(b64[-8:]) == SENTINEL64).all()), "%s: out64 guards" % case.name
        got64 = b64[8:-8].reshape(case.rows, case.cols)
    return got[1:case.rows + 1, :case.cols], got64


def same_bits(got, want, what):
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %r want %r" % (
        what, bad.size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def check(eng, case, slabs, pool, want64, what):
    dev, img = lay_out(case, slabs, pool)
    out, out64 = call_reduce(eng, case, dev)
    same_bits(out, want64.astype(np.float32), "%s %s out" % (case.name, what))
    if case.out64:
        same_bits(out64, want64, "%s %s out64" % (case.name, what))
    assert torch.equal(dev.view(torch.int32), torch.from_numpy(img).view(torch.int32).cuda()), "%s: the slabs changed" % case.name
    return dev, out, out64


# ---- which form ran: the library's own report, one child process for the table ----
_CHILD = r"""
import sys, os, torch
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import test_gpu_reduce as T
from nn_fac_amd.engine import get_engine
eng = get_engine("cuda:0")
pool = torch.zeros(T.POOL_FLOATS + 4, device="cuda")
for name, case in T.CASES.items():
    sys.stderr.write("[case] %s\n" % name)
    sys.stderr.flush()
    dev = T.aligned(pool)[case.align:case.align + case.nslab * case.stride]
    T.call_reduce(eng, case, dev, guards=False)      # (the forms only: the parent looks at the values and the sentinels)
print("done")
"""


def parse_reduce(stderr):
    """{case name: [{key: value}]} from the "[nnf reduce]" lines behind each "[case]" line."""
    out, cur = {}, None
    for line in stderr.splitlines():
        if line.startswith("[case] "):
            cur = line[7:].strip()
            out[cur] = []
        elif line.startswith("[nnf reduce] ") and cur is not None:
            out[cur].append(dict(kv.split("=", 1) for kv in line[13:].split()))
    return out


@pytest.fixture(scope="module")
def reported(built_lib):
    p = subprocess.run([sys.executable, "-c", _CHILD], env=dict(os.environ, NNF_REDUCE_DEBUG="1"), capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert p.returncode == 0 and "done" in p.stdout, p.stderr[-3000:]
    return parse_reduce(p.stderr)


@pytest.mark.gpu
def test_reduce_table(reported):
    """Every case runs the form it is listed under, with the workgroups of the restated plan: one report line per call."""
    assert list(reported) == list(CASES)
    for name, case in CASES.items():
        assert len(reported[name]) == 1, (name, reported[name])
        kv = reported[name][0]
        form, blocks = plan(case.rows, case.cols, case.nslab, case.lds, case.stride, case.align, case.out64)
        assert form == case.form, (name, form)
        assert (kv["form"], int(kv["blocks"]), kv["set"], kv["block0"]) == (form, blocks, "0/1", "0"), (name, kv)
        assert (int(kv["rows"]), int(kv["cols"]), int(kv["nslab"]), int(kv["lds"]), int(kv["ldo"]), int(kv["out64"])) == (
            case.rows, case.cols, case.nslab, case.lds, case.cols + LDO_PAD, int(case.out64)), (name, kv)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_reduce_bits(name, reported, eng, pool):
    case = CASES[name]
    form = reported[name][0]["form"]
    assert form == case.form
    seed = list(CASES).index(name)
    # exact data: the reference is integer arithmetic
    slabs, k_sum = exact_data(case, seed)
    want64 = k_sum.astype(np.float64) * 2.0 ** -20
    assert (want64 * 2.0 ** 20 == k_sum).all()
    if case.nonfinite:
        for row, col, put, expect in nonfinite_spots(case):
            for s, v in put.items():
                slabs[s, row, col] = v
            want64[row, col] = expect
        # (np.nan and the NaN a sum gives differ in sign or payload: compare these four by kind, all others by bits)
        dev, img = lay_out(case, slabs, pool)
        out, out64 = call_reduce(eng, case, dev)
        for got, want in ((out, want64.astype(np.float32)),) + (((out64, want64),) if case.out64 else ()):
            for row, col, _, expect in nonfinite_spots(case):
                g = got[row, col]
                assert np.isnan(g) if np.isnan(expect) else g == expect, (name, row, col, g, expect)
                got[row, col] = want[row, col] = 0
            same_bits(got, want, "%s non-finite, every other output" % name)
        return
    _, first, first64 = check(eng, case, slabs, pool, want64, "exact")
    # the order of the sums: the restated order of the form that ran; two calls give the same bits
    oslabs = order_data(case, 1000 + seed)
    want_o = summed(oslabs, form)
    dev, out, out64 = check(eng, case, oslabs, pool, want_o, "order")
    if case.out64:                      # the set on which most sums depend on the order, where an output can show it
        wide = order_data(case, 2000 + seed, span=30.0)
        check(eng, case, wide, pool, summed(wide, form), "order, 60 binades")
        dev, out, out64 = check(eng, case, oslabs, pool, want_o, "order")
    again, again64 = call_reduce(eng, case, dev)
    same_bits(again, out, "%s second call" % name)
    if case.out64:
        same_bits(again64, out64, "%s second call out64" % name)
    # and the first data again, right behind a call on other data
    _, back, back64 = check(eng, case, slabs, pool, want64, "exact, after other data")
    same_bits(back, first, "%s exact twice" % name)


# ---- nnf_sum_f64 ----
SUM_COUNTS = [1, 255, 256, 257, 2047, 2048, 2049, 4097, 100003]


def call_sum(eng, part, count, scale, status=0):
    buf = sentinels((3,), torch.float64)
    rc = eng.lib.nnf_sum_f64(eng.ctx, part.data_ptr() if part is not None else None, count, scale, buf[1:].data_ptr(), eng._stream())
    assert rc == status
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert bits(got)[0] == SENTINEL64 and bits(got)[2] == SENTINEL64 and (status == 0 or bits(got)[1] == SENTINEL64)
    return got[1:2]


@pytest.mark.gpu
@pytest.mark.parametrize("count", SUM_COUNTS)
def test_sum_f64_bits(count, eng):
    """Doubles k * 2^-30, |k| < 2^30: the sum of 100003 of them has at most 47 bits, times 3 at most 49 -- exact in any order, so
    the reference is the int64 sum.  A NaN in the last entry gives NaN; a NaN behind the last entry is not read into the sum."""
    rng = np.random.default_rng(count)
    k = rng.integers(-(2 ** 30) + 1, 2 ** 30, size=count, dtype=np.int64)
    assert count * 2 ** 30 * 3 < 2 ** 53
    host = np.concatenate([k.astype(np.float64) * 2.0 ** -30, [np.nan]])
    part = torch.from_numpy(host).cuda()
    for scale in (1.0, 0.5, 3.0):
        want = np.array([float(k.sum()) * 2.0 ** -30 * scale])
        same_bits(call_sum(eng, part, count, scale), want, "sum of %d, scale %r" % (count, scale))
    assert torch.equal(part.view(torch.int64), torch.from_numpy(host).view(torch.int64).cuda())
    assert np.isnan(call_sum(eng, part, count + 1, 1.0)[0])
    for at in {0, count // 2, count - 1}:
        poisoned = part.clone()
        poisoned[at] = float("nan")
        assert np.isnan(call_sum(eng, poisoned, count, 3.0)[0]), at


# ---- refusals ----
@pytest.mark.gpu
def test_refusals_launch_nothing(eng, pool):
    """NNF_ERR_ARG, and the outputs keep their sentinels (call_reduce and call_sum look at every one of them)."""
    ok = _case(7, 300, 3, "par2", out64=True)
    dev = aligned(pool)[:ok.nslab * ok.stride]
    dev.zero_()
    bad = [ok._replace(nslab=0), ok._replace(rows=0), ok._replace(cols=0), ok._replace(lds=ok.cols - 1),
           ok._replace(stride=(ok.rows - 1) * ok.lds + ok.cols - 1), ok._replace(nslab=-1)]
    for case in bad:
        out, out64 = call_reduce(eng, case, dev, status=NNF_ERR_ARG)
        assert (bits(out) == SENTINEL32).all() and (bits(out64) == SENTINEL64).all(), case
    lib, st = eng.lib, eng._stream()
    buf, buf64 = sentinels((ok.rows + 2, ok.cols + LDO_PAD), torch.float32), sentinels((ok.rows * ok.cols,), torch.float64)
    args = lambda **kw: [kw.get(k, v) for k, v in (("ctx", eng.ctx), ("slabs", dev.data_ptr()), ("nslab", ok.nslab), ("stride", ok.stride),
                                                   ("rows", ok.rows), ("cols", ok.cols), ("lds", ok.lds), ("out", buf.data_ptr()),
                                                   ("ldo", ok.cols + LDO_PAD), ("out64", buf64.data_ptr()), ("st", st))]
    for kw in (dict(ctx=None), dict(slabs=None), dict(out=None), dict(rows=0), dict(cols=0), dict(rows=-3), dict(ldo=ok.cols - 1)):
        assert lib.nnf_reduce_slabs_f32(*args(**kw)) == NNF_ERR_ARG, kw
    torch.cuda.synchronize()
    assert (buf.view(torch.int32) == SENTINEL32).all() and (buf64.view(torch.int64) == SENTINEL64).all()
    assert lib.nnf_reduce_slabs_f32(*args(out64=None)) == 0          # (out64 alone may be null)
    part = torch.ones(4, dtype=torch.float64, device="cuda")
    call_sum(eng, part, 0, 1.0, status=NNF_ERR_ARG)
    call_sum(eng, part, -1, 1.0, status=NNF_ERR_ARG)
    call_sum(eng, None, 4, 1.0, status=NNF_ERR_ARG)
    assert lib.nnf_sum_f64(None, part.data_ptr(), 4, 1.0, part.data_ptr(), st) == NNF_ERR_ARG
    assert lib.nnf_sum_f64(eng.ctx, part.data_ptr(), 4, 1.0, None, st) == NNF_ERR_ARG
    torch.cuda.synchronize()
    assert (part == 1.0).all()
