"""The fused-grid plan of a cross product with the Gram of its factor riding in the launch (nnf_plan_rider, k_stream_plan.h),
through tools/nnf_plan.cpp on the CPU: the rider starts where the cross product's grid ends, the launch is the sum of the two
grids, the workspace the sum of the two carves (the second on the cursor's 256-byte boundary), and both plans are the ones the
calls of their own take."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GIB = 1 << 30
CUS = 256

# (name, m, n, r): config B, the three unfoldings' shape of config D (500^3, rank 30), config E's row block and whole
SHAPES = [("B", 100000, 2000, 50), ("D-unfolding", 500, 250000, 30), ("E-block", 125000, 4000, 100), ("E", 1000000, 4000, 100)]


@pytest.fixture(scope="module")
def plan_tool():
    tmp = tempfile.mkdtemp(prefix="nnf_plan_fused_")
    exe = os.path.join(tmp, "nnf_plan")
    subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-I", os.path.join(ROOT, "nn_fac_amd", "csrc"),
                    os.path.join(ROOT, "tools", "nnf_plan.cpp"), "-o", exe], check=True)
    return exe


def ask(tool, *lines):
    p = subprocess.run([tool], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True)
    out = p.stdout.splitlines()
    assert len(out) == len(lines), p.stdout
    return [dict(kv.split("=", 1) for kv in re.findall(r"\S+=\S+", l)) for l in out]


def rup(a, b):
    return (a + b - 1) // b * b


@pytest.mark.parametrize("name,m,n,r", SHAPES, ids=[s[0] for s in SHAPES])
@pytest.mark.parametrize("which", ["xty", "xht"])
def test_rider_grid_and_carve_are_the_sums(plan_tool, which, name, m, n, r, ws=GIB):
    K = m if which == "xty" else n
    head = f"{CUS} {m} {n} {r} {n} 0 {ws}"
    fused, main, gram = ask(plan_tool, f"{which}_gram {head}", f"{which} {head}", f"gram {CUS} {K} {K} {r} {K} 0 {ws}")
    if name == "D-unfolding":
        # 500 x 250000 at rank 30: the Gram of the 500-long factor is one workgroup without slabs, and X H^T of a rank <= 32 is
        # the LDS-staged kernel -- neither takes a rider, the launch is the cross product's own
        assert fused["rides"] == "0" and fused["rider_grid"] == "0" and fused["rider_bytes"] == "0"
        assert fused["grid"] == fused["main_grid"] and fused["ws_bytes"] == fused["main_bytes"]
        assert which == "xht" or int(fused["main_grid"]) == int(main["grid"])
        return
    assert fused["rides"] == "1", fused
    main_grid = int(main["grid"])
    if which == "xty":
        main_bytes = int(main["nsplit"]) * r * rup(n, 4) * 4
    else:   # the k-split tail's slabs: parts x r x (the rows behind the last whole round, in fours)
        slots = main_grid
        tail_ld = rup(m - 64 * (int(main["nth"]) - 1) * slots, 4) if int(main["tail_parts"]) else 0
        main_bytes = int(main["tail_parts"]) * r * tail_ld * 4
    gram_bytes = int(gram["ws_bytes"])
    assert gram["form"] == "slabs" and gram_bytes == int(gram["nsplit"]) * r * r * 4
    # the Gram rides with the plan of its own call
    assert (fused["gram_nsplit"], fused["gram_kps"], int(fused["gram_bytes"])) == (gram["nsplit"], gram["kps"], gram_bytes)
    # the rider starts where the cross product's grid ends; the launch is the sum of both grids
    assert int(fused["main_grid"]) == main_grid
    assert int(fused["rider_offset"]) == main_grid
    assert int(fused["rider_grid"]) == int(gram["nsplit"])
    assert int(fused["grid"]) == main_grid + int(gram["nsplit"])
    # the workspace is the sum of both carves, the Gram's on the next 256-byte boundary behind the cross product's
    assert int(fused["main_bytes"]) == main_bytes and int(fused["rider_bytes"]) == gram_bytes
    assert int(fused["rider_ws_off"]) == rup(main_bytes, 256)
    assert int(fused["ws_bytes"]) == rup(main_bytes, 256) + gram_bytes


def test_no_rider_where_the_gram_has_no_slabs_or_no_room(plan_tool):
    # K <= 1024 with a contiguous G: the Gram is one workgroup writing G itself (small / single) -- the two run apart
    small, = ask(plan_tool, f"xty_gram {CUS} 1000 2000 50 2000 0 {GIB}")
    assert small["rides"] == "0" and small["rider_grid"] == "0" and small["grid"] == small["main_grid"]
    # ranks above 128 (rank passes) and the LDS-staged X H^T of ranks <= 32
    big, lds = ask(plan_tool, f"xty_gram {CUS} 100000 2000 129 2000 0 {GIB}", f"xht_gram {CUS} 100000 2000 32 2000 0 {GIB}")
    assert big["rides"] == "0" and lds["rides"] == "0"
    # a workspace that holds either carve but not both: apart, with the plans unchanged
    both, = ask(plan_tool, f"xty_gram {CUS} 100000 2000 50 2000 0 {GIB}")
    tight = int(both["ws_bytes"]) - 256
    t, main = ask(plan_tool, f"xty_gram {CUS} 100000 2000 50 2000 0 {tight}", f"xty {CUS} 100000 2000 50 2000 0 {tight}")
    assert t["rides"] == "0" and int(t["main_grid"]) == int(main["grid"]) == int(both["main_grid"])
