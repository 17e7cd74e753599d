"""The measurement panda_poly_sum_of_products stands on.  Two expressions over BN254 Fr columns of generated data:
  gate  q_L a + q_R b + q_M a b + q_O c + q_C                      8 columns, 5 terms, 10 factors (12 field products per element)
  perm  Z[i+1] a b c - Z[i] d e f + alpha l Z a d                  8 columns, 3 terms of degree 4, one rotation
each timed as
  arm M: a device-to-device panda_memcpy that moves the bytes the call reads and writes (columns + 1 vectors of n x 32 bytes of traffic,
         so half of that copied: a copy reads and writes every byte), followed by a synchronise -- the stream floor;
  arm F: the fused call;
  arm C: the same expression through a chain of panda_debug_field_op calls (one launch per binary operation, a wire conversion each way
         and a temporary in device memory per intermediate; the rotation as two device-to-device copies) -- the only way a caller had;
  arm m: arm M again (the A/A of the baseline: its run-to-run spread in the same alternation).
Every asynchronous arm is synchronised before the clock stops (the library calls end in their own synchronise, the copies are followed
by one).  Before anything is timed, at up to --verify-max elements, the fused output is compared byte for byte with the chain's.  Every
shape is warmed up, the arms alternated --alternations times, each arm timed over enough calls to last --min-seconds.  Milliseconds per
call.  One JSON line per configuration, then a table with the ratios to the copy and to the chain.

usage: sum_of_products_bench.py [--sizes n,...] [--alternations N] [--min-seconds S] [--out FILE] [--verify-max ELEMS]"""
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

DEFAULT_SIZES = "65536,1048576,16777216,1048579"
ARMS = "MFCm"
OP_ADD, OP_SUB, OP_MUL = 0, 1, 2
FIELD, FIELD_ID = 0, 1  # BN254 Fr: the library's field number and panda_debug_field_op's field id
W = 1 << 256
R_BN254 = 21888242871839275222246405745257275088548364400416034343698204186575808495617
ALPHA = 0x1234567


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


# (coefficient, [(column, rotation), ...]) and the chain that computes the same: a list of steps on named buffers
EXPRESSIONS = {
    "gate": {"columns": 8,
             "terms": [(1, [(0, 0), (5, 0)]), (1, [(1, 0), (6, 0)]), (1, [(2, 0), (5, 0), (6, 0)]), (1, [(3, 0), (7, 0)]), (1, [(4, 0)])],
             # t1 = qL a; t2 = qR b; t1 += t2; t2 = qM a; t2 *= b; t1 += t2; t2 = qO c; t1 += t2; out = t1 + qC
             "chain": [(OP_MUL, "t1", 0, 5), (OP_MUL, "t2", 1, 6), (OP_ADD, "t1", "t1", "t2"), (OP_MUL, "t2", 2, 5), (OP_MUL, "t2", "t2", 6),
                       (OP_ADD, "t1", "t1", "t2"), (OP_MUL, "t2", 3, 7), (OP_ADD, "t1", "t1", "t2"), (OP_ADD, "out", "t1", 4)]},
    "perm": {"columns": 8,
             "terms": [(1, [(0, 1), (1, 0), (2, 0), (3, 0)]), (R_BN254 - 1, [(0, 0), (4, 0), (5, 0), (6, 0)]), (ALPHA, [(7, 0), (0, 0), (1, 0), (4, 0)])],
             # zr = Z rotated by one (two copies); t1 = zr a b c; t2 = Z d e f; t1 -= t2; t2 = l Z a d alpha; out = t1 + t2
             "chain": [("rot", "zr", 0, 1), (OP_MUL, "t1", "zr", 1), (OP_MUL, "t1", "t1", 2), (OP_MUL, "t1", "t1", 3), (OP_MUL, "t2", 0, 4),
                       (OP_MUL, "t2", "t2", 5), (OP_MUL, "t2", "t2", 6), (OP_SUB, "t1", "t1", "t2"), (OP_MUL, "t2", 7, 0), (OP_MUL, "t2", "t2", 1),
                       (OP_MUL, "t2", "t2", 4), (OP_MUL, "t2", "t2", "alpha"), (OP_ADD, "out", "t1", "t2")]},
}


def table(recs):
    lines = ["expr  n           traffic MiB | M copy (min / med / max ms)   | m med    spread  | fused ms   x copy | chain ms   x copy | chain / fused | fused G elem/s  chain launches"]
    for r in recs:
        med = r["median_ms"]
        lines.append("%-5s %-10d %12.1f | %8.4f /%8.4f /%8.4f | %8.4f %7.4f | %9.4f %7.2f | %9.4f %7.2f | %13.2f | %14.3f %15d" % (
            r["expression"], r["n"], r["traffic_bytes"] / 2**20, *r["M_min_med_max"], med["m"], r["baseline_spread_ms"], med["F"], r["fused_to_copy"],
            med["C"], r["chain_to_copy"], r["chain_to_fused"], r["fused_gelem_per_s"], r["chain_launches"]))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=DEFAULT_SIZES)
    ap.add_argument("--expressions", default="gate,perm")
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--min-seconds", type=float, default=0.2)
    ap.add_argument("--out")
    ap.add_argument("--verify-max", type=int, default=1 << 24)
    a = ap.parse_args()
    import numpy as np
    from gpu_util import NULL_STREAM, DeviceBuffer
    from panda_amd import gpu_manager as pgm
    lib = ffi.load()
    gm = pgm.PandaGpuManager(0)
    out_file = open(a.out, "a") if a.out else None
    recs = []
    name = device_name()
    try:
        for n in (int(s) for s in a.sizes.split(",")):
            nbytes = n * 32
            cols = [DeviceBuffer(nbytes) for _ in range(8)]
            extra = {k: DeviceBuffer(nbytes) for k in ("t1", "t2", "zr", "alpha", "out", "fused")}
            vectors = max(spec["columns"] + 1 for spec in EXPRESSIONS.values())  # the widest expression's traffic: its columns and the output
            copy_src, copy_dst = DeviceBuffer(vectors * nbytes // 2 + 32), DeviceBuffer(vectors * nbytes // 2 + 32)
            stream = gm.exec_stream.raw
            try:
                for k, d in enumerate(cols):
                    ffi.check(lib.panda_gen_scalars(FIELD, 0x50B + 16 * k + n, 0, n, d.ptr, NULL_STREAM), "gen")
                ffi.check(lib.panda_gen_scalars(FIELD, 0x60B + n, 0, vectors * n // 2 + 1, copy_src.ptr, NULL_STREAM), "gen")
                ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")
                alpha = np.ascontiguousarray(np.broadcast_to(wire(ALPHA), (min(n, 1 << 16), 8)))
                for off in range(0, n, len(alpha)):  # the chain's constant column, filled once outside the timed region
                    cnt = min(len(alpha), n - off)
                    ffi.check(lib.panda_memcpy(C.c_void_p(extra["alpha"].ptr.value + off * 32), C.c_void_p(alpha.ctypes.data), cnt * 32), "copy")
                for ename in a.expressions.split(","):
                    spec = EXPRESSIONS[ename]
                    terms = spec["terms"]
                    traffic = (spec["columns"] + 1) * nbytes
                    ptrs = (C.c_void_p * 8)(*[d.ptr.value for d in cols])
                    coeffs = np.ascontiguousarray(np.stack([wire(k) for k, _ in terms]))
                    degrees = (C.c_uint * len(terms))(*[len(fs) for _, fs in terms])
                    flat = [f for _, fs in terms for f in fs]
                    factors = (ffi.SopFactor * len(flat))(*[ffi.SopFactor(c, r) for c, r in flat])
                    expr = ffi.SopExpression(ptrs, C.c_void_p(coeffs.ctypes.data), degrees, factors, None, 8, len(terms), 0, ffi.SOP_SCALE_NONE)

                    def buf(x):
                        return cols[x].ptr if isinstance(x, int) else extra[x].ptr

                    def run_copy():  # a device-to-device copy returns before it has run: the arm ends in a synchronise, like the library's calls
                        ffi.check(lib.panda_memcpy(copy_dst.ptr, copy_src.ptr, traffic // 2), "copy")
                        ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")

                    def run_fused():
                        ffi.check(lib.panda_poly_sum_of_products(FIELD, C.byref(expr), extra["fused"].ptr, n, 1, stream), "sum_of_products")

                    def run_chain():
                        for op, dst, x, y in spec["chain"]:
                            if op == "rot":  # dst[i] = x[(i + y) mod n]
                                ffi.check(lib.panda_memcpy(buf(dst), C.c_void_p(buf(x).value + y * 32), (n - y) * 32), "copy")
                                ffi.check(lib.panda_memcpy(C.c_void_p(buf(dst).value + (n - y) * 32), buf(x), y * 32), "copy")
                                ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")
                            else:
                                ffi.check(lib.panda_debug_field_op(FIELD_ID, op, buf(dst), buf(x), buf(y), n, stream), "field_op")

                    run = {"M": run_copy, "F": run_fused, "C": run_chain, "m": run_copy}
                    verified = n <= a.verify_max
                    if verified:
                        run_fused()
                        run_chain()
                        if not np.array_equal(extra["fused"].to_host(np.uint32), extra["out"].to_host(np.uint32)):
                            raise SystemExit(f"{ename} at n = {n}: the fused result differs from the chain's")
                    reps = {}
                    for arm in ARMS:  # warm-up of every shape
                        run[arm]()
                        t0 = time.perf_counter()
                        run[arm]()
                        reps[arm] = max(1, int(a.min_seconds / max(time.perf_counter() - t0, 1e-6)) + 1)
                    ms = {arm: [] for arm in ARMS}
                    for _ in range(a.alternations):
                        for arm in ARMS:
                            t0 = time.perf_counter()
                            for _ in range(reps[arm]):
                                run[arm]()
                            ms[arm].append((time.perf_counter() - t0) / reps[arm] * 1e3)
                    med = {arm: statistics.median(ms[arm]) for arm in ARMS}
                    spread = max(max(ms["M"]) - min(ms["M"]), max(ms["m"]) - min(ms["m"]), abs(med["M"] - med["m"]))
                    tile, launches = C.c_uint(0), C.c_uint(0)
                    ffi.check(lib.panda_poly_sum_of_products_plan(n, 1, C.byref(tile), C.byref(launches)), "plan")
                    rec = {"expression": ename, "field": FIELD, "n": n, "columns": spec["columns"], "terms": len(terms), "factors": len(flat),
                           "traffic_bytes": traffic, "device": name, "tile": tile.value, "launches": launches.value, "verified": verified,
                           "chain_launches": sum(2 if s[0] == "rot" else 1 for s in spec["chain"]), "calls_per_repetition": reps,
                           "per_call_ms": {arm: [round(v, 5) for v in ms[arm]] for arm in ARMS},
                           "median_ms": {arm: round(med[arm], 5) for arm in ARMS},
                           "M_min_med_max": [round(min(ms["M"]), 5), round(med["M"], 5), round(max(ms["M"]), 5)],
                           "baseline_spread_ms": round(spread, 5),
                           "fused_to_copy": round(med["F"] / med["M"], 4), "chain_to_copy": round(med["C"] / med["M"], 4),
                           "chain_to_fused": round(med["C"] / med["F"], 4),
                           "copy_gb_per_s": round(traffic / med["M"] / 1e6, 1), "fused_gelem_per_s": round(n / med["F"] / 1e6, 3)}
                    recs.append(rec)
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if out_file:
                        out_file.write(line + "\n")
                        out_file.flush()
            finally:
                for b in cols + list(extra.values()) + [copy_src, copy_dst]:
                    b.free()
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
