#!/usr/bin/env python3
"""Times the projected-gradient core update of NTD on cores of order 4 and 5: the Kronecker-merged route through the
three-mode entry (nnf_ntd_core_pg_f32) against the native n-mode entry (nnf_ntd_core_pgn_f32).

    python tools/time_ntd_core.py [--reps 20] [--warmup 3] [--parts abc] [--out FILE]

Parts
  a   the core update alone (max_iter = 300, delta = 0: all 300 steps run), merged against native, on cores both take;
      the merged Gram (torch.kron) is built outside the timed region.
  b   the native entry alone on cores only it takes: (8,8,12,12) multi, (2,2,64,64) ws, (2,100,100,3) ws with the Gram
      images in the workspace.
  c   one compute_ntd HALS iteration on a 60^4 tensor with ranks (8,8,8,8), default route against NNF_NTD_CORE_NATIVE=1.

HIP events around the call, medians of `reps` calls after `warmup` calls; where two routes are compared they are interleaved
call by call in one process (the same kernel moves by several per cent with the state of the chip: only interleaved medians
compare).  One JSON line per case on stdout; --out writes the whole table with the command and the commit.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOTH = [(8, 8, 8, 8), (6, 6, 10, 10), (16, 4, 8, 8), (4, 4, 4, 4, 4)]
NATIVE_ONLY = [(8, 8, 12, 12), (2, 2, 64, 64), (2, 100, 100, 3)]
MAX_ITER = 300


def problem(torch, dims, scale=0.3):
    """Grams of scale * rand factors (5 d + 3 rows), MtX of a random non-negative core pushed through them, a random start."""
    g = torch.Generator(device="cuda").manual_seed(sum(dims))
    M = []
    for d in dims:
        F = scale * torch.rand(5 * d + 3, d, device="cuda", generator=g, dtype=torch.float64)
        M.append(F.t() @ F)
    x = torch.rand(*dims, device="cuda", generator=g, dtype=torch.float64)
    for i, m in enumerate(M):
        x = torch.movedim(torch.tensordot(m, x, dims=([1], [i])), 0, i)
    core0 = torch.rand(*dims, device="cuda", generator=g, dtype=torch.float64).float().contiguous()
    return [m.float().contiguous() for m in M], x.float().contiguous(), core0


def timed(torch, calls, reps, warmup, before=None):
    """calls: {name: callable}; interleaved name by name; `before` runs untimed ahead of every call.  Medians in us."""
    stream = torch.cuda.current_stream()
    times = {nm: [] for nm in calls}
    for it in range(warmup + reps):
        for nm, fn in calls.items():
            if before:
                before(nm)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            if it >= warmup:
                times[nm].append(a.elapsed_time(b) * 1e3)
    out = {}
    for nm, t in times.items():
        out[nm + "_us"] = round(statistics.median(t), 1)
        out[nm + "_min_us"] = round(min(t), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--out", default=None, help="write the table (command, commit, cases) to this JSON file")
    args = ap.parse_args()

    import torch
    from nn_fac_amd.engine import get_engine
    eng = get_engine("cuda:0")
    rows = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        rows.append(rec)

    def core_case(dims, merged):
        M, MtX, core0 = problem(torch, dims)
        work = torch.empty_like(core0)
        status = torch.empty(6, dtype=torch.float64, device="cuda")
        calls = {"native": lambda: eng.ntd_core_pgn(work, MtX, M, 0.0, 0.0, MAX_ITER, 1.0, status=status)}
        if merged:
            tail = 1
            for d in dims[2:]:
                tail *= d
            Mk = M[2]
            for g in M[3:]:
                Mk = torch.kron(Mk.contiguous(), g.contiguous())
            d3 = (dims[0], dims[1], tail)
            w3, x3 = work.view(d3), MtX.view(d3)
            calls = {"merged": lambda: eng.ntd_core_pg(w3, x3, [M[0], M[1], Mk], 0.0, 0.0, MAX_ITER, 1.0, status=status), **calls}
        rec = {"part": "a" if merged else "b", "dims": list(dims), "S": core0.numel(), "max_iter": MAX_ITER, "delta": 0,
               "reps": args.reps}
        rec.update(timed(torch, calls, args.reps, args.warmup, before=lambda nm: work.copy_(core0)))
        st = status.cpu().tolist()
        rec["steps_run"], rec["timed_out"] = int(st[0]), bool(st[5])
        if merged:
            rec["merged_over_native"] = round(rec["merged_us"] / rec["native_us"], 3)
        emit(rec)

    if "a" in args.parts:
        for dims in BOTH:
            core_case(dims, True)
    if "b" in args.parts:
        for dims in NATIVE_ONLY:
            core_case(dims, False)
    if "c" in args.parts:
        from nn_fac_amd.ntd import compute_ntd
        shape, ranks = (60, 60, 60, 60), (8, 8, 8, 8)
        g = torch.Generator(device="cuda").manual_seed(1)
        T = torch.rand(*shape, device="cuda", generator=g)
        C0 = (torch.rand(*ranks, device="cuda", generator=g) + 0.05).contiguous()
        F0 = [(torch.rand(s, q, device="cuda", generator=g) + 0.05).contiguous() for s, q in zip(shape, ranks)]
        kw = dict(n_iter_max=1, tol=0, update_rule="hals", deterministic=True, sparsity_coefficients=[None] * 5,
                  normalize=[False] * 5)

        def run(native):
            def f():
                if native:
                    os.environ["NNF_NTD_CORE_NATIVE"] = "1"
                else:
                    os.environ.pop("NNF_NTD_CORE_NATIVE", None)
                compute_ntd(T, list(ranks), C0, F0, **kw)
            return f
        saved = os.environ.get("NNF_NTD_CORE_NATIVE")
        rec = {"part": "c", "shape": list(shape), "ranks": list(ranks), "what": "one compute_ntd HALS iteration", "reps": args.reps}
        rec.update(timed(torch, {"merged": run(False), "native": run(True)}, args.reps, args.warmup))
        rec["merged_over_native"] = round(rec["merged_us"] / rec["native_us"], 3)
        os.environ.pop("NNF_NTD_CORE_NATIVE", None)
        if saved is not None:
            os.environ["NNF_NTD_CORE_NATIVE"] = saved
        emit(rec)

    if args.out:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
        except OSError:
            commit = None
        doc = {"what": "NTD core update on cores of order 4 and 5, whole call on the stream (HIP events), medians of %d after %d "
                       "warm-up calls, microseconds; merged: trailing modes merged, Kronecker Gram, nnf_ntd_core_pg_f32; native: "
                       "nnf_ntd_core_pgn_f32; routes interleaved call by call" % (args.reps, args.warmup),
               "command": "python tools/time_ntd_core.py " + " ".join(sys.argv[1:]), "commit": commit,
               "device": torch.cuda.get_device_name(0), "cases": rows}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
