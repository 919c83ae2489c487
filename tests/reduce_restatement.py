"""The slab reduction behind every split launch (nn_fac_amd/csrc/k_reduce.hip), restated in plain Python from its rule: which
form a set of slabs takes with how many workgroups (nnf_plan_reduce_set, k_stream_plan.h) and the ORDER in which each form adds
the slabs in fp64.  Nothing here is copied from the code, and nothing here runs the code: tests/test_reduce_plan.py compares
plan() with the library's own plan function through tools/nnf_plan.cpp, tests/test_gpu_reduce.py compares summed() with the
device bit for bit.  A change of the forms, the thresholds or the summation order changes this file in the same commit."""
import numpy as np

FORMS = ("plain", "vec4", "par2", "par4", "par8", "par16")
PARTS = {"par2": 2, "par4": 4, "par8": 8, "par16": 16}


def cdiv(a, b):
    return -(-a // b)


def plan(rows, cols, nslab, lds, stride, align, out64):
    """(form, workgroups) of one set: rows x cols sums of nslab slabs at row pitch lds, `stride` floats from slab to slab, the
    first slab `align` floats past a 16-byte boundary, out64: the fp64 sums are asked for as well.
      parP  -- P = 2^lg threads per element, where few elements leave the chip idle: rows * cols < 2^19 and at least two
               slabs; lg is the largest l <= 4 with rows * cols < 2^(20 - l) and nslab >= 2^l; 256 / P elements per workgroup;
      vec4  -- four columns per thread (16-byte loads): no out64, lds and stride multiples of 4, 16-byte aligned slabs and
               rows * cols >= 2^21; 256 quads per workgroup, at most 2048 workgroups;
      plain -- one element per thread, 256 per workgroup, at most 2048 workgroups."""
    total = rows * cols
    if total < 2 ** 19 and nslab >= 2:
        lg = max(l for l in range(1, 5) if total < 2 ** (20 - l) and nslab >= 2 ** l)
        return "par%d" % 2 ** lg, min(4096, cdiv(total, 256 >> lg))
    if not out64 and lds % 4 == 0 and stride % 4 == 0 and align % 4 == 0 and total >= 2 ** 21:
        return "vec4", min(2048, cdiv(rows * cdiv(cols, 4), 256))
    return "plain", min(2048, max(1, cdiv(total, 256)))


def summed(slabs, form):
    """The fp64 sums of slabs[s] over s (any array shape per slab) in the order the form documents: plain and vec4 add the
    slabs one after the other onto 0.0; parP cuts them into P parts of per = ceil(nslab / P) consecutive slabs -- part c holds
    [c * per, min((c + 1) * per, nslab)), possibly none -- adds each part's slabs one after the other onto 0.0, then adds the
    parts onto part 0 in part order.  The fp32 result of the device is the rounding of this sum."""
    slabs = np.asarray(slabs)
    nslab = slabs.shape[0]

    def chain(lo, hi):
        s = np.zeros(slabs.shape[1:], dtype=np.float64)
        for k in range(lo, min(hi, nslab)):
            s = s + slabs[k].astype(np.float64)
        return s

    if form in ("plain", "vec4"):
        return chain(0, nslab)
    P = PARTS[form]
    per = cdiv(nslab, P)
    t = chain(0, per)
    for c in range(1, P):
        t = t + chain(c * per, (c + 1) * per)
    return t
