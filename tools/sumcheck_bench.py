"""The measurement the sumcheck calls stand on.  BN254 Fr tables of generated data, 2^k elements each, two expressions:
  gate     eq (q_L a + q_R b + q_M a b + q_O c + q_C)     9 columns, 5 terms, 15 factors, 5 evaluation points
  spartan  eq (a b - c)                                   4 columns, 2 terms,  5 factors, 4 evaluation points
A whole k-round sumcheck (the challenges fixed in advance; a transcript would hash between the calls) timed as
  arm F: one plain panda_sumcheck_round, k - 1 fused rounds, the last panda_mle_fold;
  arm U: a plain round and a panda_mle_fold per round -- the unfused arm of the same build;
  arm M: per round one device-to-device panda_memcpy that moves the bytes arm F's call reads and writes (half of them copied: a copy
         reads and writes every byte), each followed by a synchronise as every library call ends in one;
  arm m: arm M again (the A/A of the baseline: its run-to-run spread in the same alternation).
The largest fused round alone (log_n = k with a challenge) is timed the same way against its fold + plain round and its copy, and
panda_mle_eq_table against a copy of its output bytes.  Before anything is timed the evaluations of arm F are compared byte for byte with
arm U's, round by round.  Every shape is warmed up, the arms alternated --alternations times, each arm timed over enough runs to last
--min-seconds.  Milliseconds per run.  One JSON line per configuration, then a table.

usage: sumcheck_bench.py [--log-sizes k,...] [--expressions gate,spartan] [--alternations N] [--min-seconds S] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from panda_amd import gpu_ffi as ffi  # noqa: E402

FIELD = 0
W = 1 << 256
R_BN254 = 21888242871839275222246405745257275088548364400416034343698204186575808495617
ARMS = "MFUm"
EXPRESSIONS = {
    "gate": {"columns": 9, "n_evals": 5, "terms": [(1, [0, 1, 6]), (1, [0, 2, 7]), (1, [0, 3, 6, 7]), (1, [0, 4, 8]), (1, [0, 5])]},
    "spartan": {"columns": 4, "n_evals": 4, "terms": [(1, [0, 1, 2]), (R_BN254 - 1, [0, 3])]},
}


def device_name():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return f"{p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs)"
    except Exception as e:  # noqa: BLE001
        return f"unknown ({type(e).__name__})"


def wire(v):
    import numpy as np
    return np.frombuffer((v % R_BN254 * W % R_BN254).to_bytes(32, "little"), np.uint32)


def measure(run, alternations, min_seconds):
    """run: {arm: callable} -> per-arm lists of ms per run, alternated"""
    reps = {}
    for arm in ARMS:
        run[arm]()
        t0 = time.perf_counter()
        run[arm]()
        reps[arm] = max(1, int(min_seconds / max(time.perf_counter() - t0, 1e-6)) + 1)
    ms = {arm: [] for arm in ARMS}
    for _ in range(alternations):
        for arm in ARMS:
            t0 = time.perf_counter()
            for _ in range(reps[arm]):
                run[arm]()
            ms[arm].append((time.perf_counter() - t0) / reps[arm] * 1e3)
    return ms


def summary(ms):
    med = {arm: statistics.median(ms[arm]) for arm in ARMS}
    spread = max(max(ms["M"]) - min(ms["M"]), max(ms["m"]) - min(ms["m"]), abs(med["M"] - med["m"]))
    return {"per_run_ms": {arm: [round(v, 5) for v in ms[arm]] for arm in ARMS}, "median_ms": {arm: round(med[arm], 5) for arm in ARMS},
            "copy_spread_ms": round(spread, 5), "fused_to_copy": round(med["F"] / med["M"], 4), "unfused_to_copy": round(med["U"] / med["M"], 4),
            "unfused_to_fused": round(med["U"] / med["F"], 4), "fused_faster_beyond_spread": bool(med["U"] - med["F"] > spread)}


def table(recs):
    lines = ["what       expr     k   traffic MiB | copy M ms   m ms     spread | fused ms  x copy | unfused ms  x copy | unfused / fused  fused wins"]
    for r in recs:
        med = r["median_ms"]
        lines.append("%-10s %-8s %-3d %11.1f | %9.4f %9.4f %7.4f | %9.4f %6.2f | %10.4f %6.2f | %15.3f  %s" % (
            r["what"], r["expression"], r["k"], r["traffic_bytes"] / 2**20, med["M"], med["m"], r["copy_spread_ms"], med["F"], r["fused_to_copy"],
            med["U"], r["unfused_to_copy"], r["unfused_to_fused"], "yes" if r["fused_faster_beyond_spread"] else "no"))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-sizes", default="16,20,24")
    ap.add_argument("--expressions", default="gate,spartan")
    ap.add_argument("--order", type=int, default=ffi.MLE_BIND_LOW)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--min-seconds", type=float, default=0.2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    from gpu_util import NULL_STREAM, DeviceBuffer
    from panda_amd import gpu_manager as pgm
    lib = ffi.load()
    gm = pgm.PandaGpuManager(0)
    out_file = open(a.out, "a") if a.out else None
    recs = []
    name = device_name()

    def emit(rec):
        recs.append(rec)
        line = json.dumps(rec)
        print(line, flush=True)
        if out_file:
            out_file.write(line + "\n")
            out_file.flush()

    try:
        for k in (int(s) for s in a.log_sizes.split(",")):
            n, stream, order = 1 << k, gm.exec_stream.raw, a.order
            for ename in a.expressions.split(","):
                spec = EXPRESSIONS[ename]
                m, terms, n_evals = spec["columns"], spec["terms"], spec["n_evals"]
                # set 0 holds the tables and is never written; the folded tables alternate between sets 1 and 2
                sets = [[DeviceBuffer(32 * n >> s) for _ in range(m)] for s in range(3)]
                copy_bytes = m * 32 * (n + n // 2) // 2
                copy_src, copy_dst = DeviceBuffer(copy_bytes + 32), DeviceBuffer(copy_bytes + 32)
                try:
                    for c, d in enumerate(sets[0]):
                        ffi.check(lib.panda_gen_scalars(FIELD, 0x5C + 16 * c + k, 0, n, d.ptr, NULL_STREAM), "gen")
                    ffi.check(lib.panda_gen_scalars(FIELD, 0x6C + k, 0, copy_bytes // 32 + 1, copy_src.ptr, NULL_STREAM), "gen")
                    ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")
                    coeffs = np.ascontiguousarray(np.stack([wire(c) for c, _ in terms]))
                    degrees = (C.c_uint * len(terms))(*[len(fs) for _, fs in terms])
                    flat = [c for _, fs in terms for c in fs]
                    factors = (ffi.SopFactor * len(flat))(*[ffi.SopFactor(c, 0) for c in flat])
                    challenges = [np.ascontiguousarray(wire(0x1234567 + 977 * j)) for j in range(k)]
                    ptrs = [(C.c_void_p * m)(*[d.ptr.value for d in s]) for s in sets]
                    exprs = [ffi.SopExpression(p, C.c_void_p(coeffs.ctypes.data), degrees, factors, None, m, len(terms), 0, ffi.SOP_SCALE_NONE) for p in ptrs]
                    evals = {arm: np.zeros((k, n_evals, 8), np.uint32) for arm in "FU"}

                    def round_call(arm, j, src, log_n, challenge=None, dst=None):
                        ffi.check(lib.panda_sumcheck_round(FIELD, C.byref(exprs[src]), log_n, order, n_evals,
                                                           None if challenge is None else C.c_void_p(challenge.ctypes.data),
                                                           None if dst is None else ptrs[dst], C.c_void_p(evals[arm][j].ctypes.data), stream), "round")

                    def fold_call(src, dst, log_n, challenge):
                        ffi.check(lib.panda_mle_fold(FIELD, ptrs[src], ptrs[dst], m, log_n, order, C.c_void_p(challenge.ctypes.data), stream), "fold")

                    def copy_call(nbytes):
                        ffi.check(lib.panda_memcpy(copy_dst.ptr, copy_src.ptr, max(nbytes // 2, 32)), "copy")
                        ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")

                    def next_set(cur):
                        return 2 if cur == 1 else 1

                    # the bytes arm F's calls move, call by call: the plain round, the fused rounds, the last fold
                    call_bytes = [m * 32 * n] + [m * 32 * ((1 << (k - j + 1)) + (1 << (k - j))) for j in range(1, k)] + [m * 32 * 3]

                    def run_fused():
                        cur = 0
                        round_call("F", 0, cur, k)
                        for j in range(1, k):
                            round_call("F", j, cur, k - j + 1, challenges[j - 1], next_set(cur))
                            cur = next_set(cur)
                        fold_call(cur, next_set(cur), 1, challenges[k - 1])

                    def run_unfused():
                        cur = 0
                        round_call("U", 0, cur, k)
                        for j in range(1, k):
                            fold_call(cur, next_set(cur), k - j + 1, challenges[j - 1])
                            cur = next_set(cur)
                            round_call("U", j, cur, k - j)
                        fold_call(cur, next_set(cur), 1, challenges[k - 1])

                    def run_copy():
                        for b in call_bytes:
                            copy_call(b)

                    run_fused()
                    run_unfused()
                    if not np.array_equal(evals["F"], evals["U"]):
                        raise SystemExit(f"{ename} at k = {k}: the fused rounds' evaluations differ from the unfused ones")
                    base = {"expression": ename, "field": FIELD, "k": k, "order": order, "columns": m, "terms": len(terms), "factors": len(flat),
                            "n_evals": n_evals, "device": name, "verified": True}
                    emit({**base, "what": "sumcheck", "traffic_bytes": sum(call_bytes), "calls": {"F": k + 1, "U": 2 * k},
                          **summary(measure({"M": run_copy, "F": run_fused, "U": run_unfused, "m": run_copy}, a.alternations, a.min_seconds))})

                    def first_fused():
                        round_call("F", 1, 0, k, challenges[0], 1)

                    def first_unfused():
                        fold_call(0, 1, k, challenges[0])
                        round_call("U", 1, 1, k - 1)

                    def first_copy():
                        copy_call(call_bytes[1])

                    emit({**base, "what": "round", "traffic_bytes": call_bytes[1], "calls": {"F": 1, "U": 2},
                          **summary(measure({"M": first_copy, "F": first_fused, "U": first_unfused, "m": first_copy}, a.alternations, a.min_seconds))})
                finally:
                    for b in [d for s in sets for d in s] + [copy_src, copy_dst]:
                        b.free()
            # the eq table against a copy of its output bytes (arm U is the call again: there is no second path)
            out, src = DeviceBuffer(32 * n), DeviceBuffer(32 * n)
            try:
                point = np.ascontiguousarray(np.stack([wire(0x7654321 + 31 * j) for j in range(k)]))

                def eq_call():
                    ffi.check(lib.panda_mle_eq_table(FIELD, C.c_void_p(point.ctypes.data), k, out.ptr, stream), "eq")

                def eq_copy():
                    ffi.check(lib.panda_memcpy(out.ptr, src.ptr, 32 * n), "copy")
                    ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")

                emit({"what": "eq_table", "expression": "-", "field": FIELD, "k": k, "device": name, "traffic_bytes": 32 * n,
                      **summary(measure({"M": eq_copy, "F": eq_call, "U": eq_call, "m": eq_copy}, a.alternations, a.min_seconds))})
            finally:
                out.free()
                src.free()
        text = table(recs)
        print(text, flush=True)
        if out_file:
            out_file.write(text + "\n")
    finally:
        if out_file:
            out_file.close()
        gm.deinit()


if __name__ == "__main__":
    main()
