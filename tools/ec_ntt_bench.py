"""The measurement panda_ec_ntt and panda_points_to_affine stand on.  Inputs are panda_gen_bases points; nothing is compared with a CPU
here (tests/test_ec_ntt.py does that): before anything is timed inverse(forward(P)) must give P back byte for byte.
  transforms   2^12, 2^16, 2^20 (--logs) for the curves 0 BN254, 1 BLS12-377, 2 BLS12-381 (--curves), arms F (forward) and I (inverse)
               alternated --alternations times, each call synchronous (it ends in a synchronise), medians in ms per call
  group ops    doublings + additions the kernels issue PER WAVE, counted from the plan, times 64 lanes: a uniform butterfly is b doublings
               and about b / 2 + 2 additions for a b-bit scalar field, a divergent one b doublings and b + 2 additions (a wave pays both for
               every bit), the first stage 2 additions, the inverse's scaling b doublings + popcount(1 / n) additions per point
  stage costs  per kernel, from a kernel trace of this tool (rocprofv3 --kernel-trace --stats -- python tools/ec_ntt_bench.py --logs 20
               --alternations 1 --skip-msm): k_stage<.., true> against k_stage<.., false>, each divided by its launches x n / 2.  Without a
               profiler, two sizes of at least 2^19 (--logs 20,22: below that a stage is one butterfly's latency, not throughput) give
               a fit: (t(2^b) / 2^(b-1) - t(2^a) / 2^(a-1)) / (b - a) is one uniform stage per butterfly, and what is left of
               t(2^a) / 2^(a-1) over its uniform stages is the six divergent ones with the first stage, the table and the normalisation.
  k_accumulate one BN254 MSM of 2^20 against precomputed tables under panda_msm_set_phase_timing(1): its bucket-accumulation time and
               2^20 x tables additions, the one point-arithmetic kernel whose ceiling is known, from the same session
  to affine    panda_points_to_affine at 2^16 and 2^20 Jacobian triples (an MSM result repeated) against arm M, one device-to-device copy
               of its traffic (triples in, affine points out; a copy reads and writes every byte, so half of them are copied)
One JSON line per record, then a table.

usage: ec_ntt_bench.py [--curves 0,1,2] [--logs 12,16,20] [--alternations N] [--once LOG] [--out FILE]"""
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

POINT = {0: 64, 1: 96, 2: 96}
R_BITS = {0: 254, 1: 253, 2: 255}
R = {0: 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001, 1: 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001,
     2: 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001}
NAME = {0: "bn254", 1: "bls12_377", 2: "bls12_381"}


def device_name():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return f"{p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs)"
    except Exception as e:  # noqa: BLE001
        return f"unknown ({type(e).__name__})"


def group_ops(curve, log_n, inverse):
    """doublings + additions issued, per wave x 64 lanes, over the whole transform"""
    n, b = 1 << log_n, R_BITS[curve]
    uniform = max(0, log_n - 6)
    stages = log_n
    mult_uniform = max(0, uniform - 1)              # the first stage multiplies by nothing
    mult_divergent = stages - uniform - (1 if uniform == 0 and stages else 0)
    ops = (n // 2) * (2 * stages + mult_uniform * (b + b / 2) + mult_divergent * 2 * b)
    if inverse and log_n:
        ops += n * (b + bin(pow(n, -1, R[curve])).count("1"))
    return ops


def alternate(run, arms, alternations):
    ms = {arm: [] for arm in arms}
    for arm in arms:
        run[arm]()
    for _ in range(alternations):
        for arm in arms:
            t0 = time.perf_counter()
            run[arm]()
            ms[arm].append((time.perf_counter() - t0) * 1e3)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="0,1,2")
    ap.add_argument("--logs", default="12,16,20")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--once", type=int, default=0, help="also run one inverse BN254 transform of this log2 size, in place, once (2^24 for the README)")
    ap.add_argument("--skip-msm", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import oracle as po
    from gpu_util import NULL_STREAM, DeviceBuffer
    from panda_amd import gpu_manager as pgm
    lib = ffi.load()
    gm = pgm.PandaGpuManager(0)
    stream = gm.exec_stream.raw
    out_file = open(a.out, "a") if a.out else None
    name = device_name()
    recs = []

    def emit(rec):
        rec["device"] = name
        recs.append(rec)
        line = json.dumps(rec)
        print(line, flush=True)
        if out_file:
            out_file.write(line + "\n")
            out_file.flush()

    def transform(curve, src, dst, log_n, direction):
        om = np.ascontiguousarray(po.root_of_unity(po.FR_OF[curve], log_n))
        ffi.check(lib.panda_ec_ntt(curve, src.ptr, dst.ptr, log_n, direction, C.c_void_p(om.ctypes.data), stream), "ec_ntt")

    try:
        curves, logs = [int(c) for c in a.curves.split(",")], [int(v) for v in a.logs.split(",")]
        for curve in curves:
            per_size = {}
            for log_n in logs:
                n = 1 << log_n
                bufs = [DeviceBuffer(n * POINT[curve]) for _ in range(3)]
                try:
                    ffi.check(lib.panda_gen_bases(curve, 0xEC, 0, n, bufs[0].ptr, NULL_STREAM), "gen")
                    ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")
                    transform(curve, bufs[0], bufs[1], log_n, 0)
                    transform(curve, bufs[1], bufs[2], log_n, 1)
                    if not np.array_equal(bufs[0].to_host(), bufs[2].to_host()):
                        raise SystemExit(f"curve {curve} 2^{log_n}: inverse(forward(P)) != P")
                    run = {"F": lambda: transform(curve, bufs[0], bufs[1], log_n, 0), "I": lambda: transform(curve, bufs[1], bufs[2], log_n, 1)}
                    ms = alternate(run, "FI", a.alternations)
                    med = {arm: statistics.median(ms[arm]) for arm in "FI"}
                    plan = [C.c_uint(0), C.c_size_t(0), C.c_uint(0)]
                    ffi.check(lib.panda_ec_ntt_plan(curve, log_n, 0, *[C.byref(v) for v in plan]), "plan")
                    per_size[log_n] = med["F"]
                    emit({"what": "ec_ntt", "curve": NAME[curve], "log_n": log_n, "launches_forward": plan[0].value, "scratch_bytes": plan[1].value,
                          "uniform_stages": plan[2].value, "per_run_ms": {k: [round(v, 4) for v in ms[k]] for k in "FI"},
                          "median_ms": {k: round(med[k], 4) for k in "FI"},
                          "group_ops_per_s": {"F": round(group_ops(curve, log_n, False) / med["F"] * 1e3), "I": round(group_ops(curve, log_n, True) / med["I"] * 1e3)}})
                finally:
                    for b in bufs:
                        b.free()
            fit = sorted(k for k in per_size if k >= 19)  # both sizes must fill the device: below 2^19 a stage is one butterfly's latency
            if len(fit) >= 2:
                lo, hi = fit[-2], fit[-1]
                per_lo, per_hi = per_size[lo] / (1 << (lo - 1)), per_size[hi] / (1 << (hi - 1))  # ms per butterfly column
                uniform = (per_hi - per_lo) / (hi - lo)
                divergent = (per_lo - (lo - 7) * uniform) / 6
                emit({"what": "stage_cost", "curve": NAME[curve], "from_logs": [lo, hi], "uniform_ns_per_butterfly": round(uniform * 1e6, 2),
                      "divergent_ns_per_butterfly": round(divergent * 1e6, 2), "ratio": round(divergent / uniform, 3) if uniform > 0 else None})
        if not a.skip_msm:
            log_n, n = 20, 1 << 20
            db, ds = DeviceBuffer(n * 64), DeviceBuffer(n * 32)
            res = np.zeros(24, np.uint32)
            try:
                ffi.check(lib.panda_gen_bases(0, 0xEC, 0, n, db.ptr, NULL_STREAM), "gen")
                ffi.check(lib.panda_gen_scalars(0, 0xED, 0, n, ds.ptr, NULL_STREAM), "gen")
                ffi.check(lib.panda_msm_precompute_bases(0, db.ptr, log_n, 0, stream), "precompute")
                tables, bits = C.c_uint(0), C.c_uint(0)
                ffi.check(lib.panda_msm_registered_info(db.ptr, C.byref(tables), C.byref(bits), None), "info")
                ffi.check(lib.panda_msm_set_phase_timing(1), "timing")
                cfg = ffi.MSMConfiguration(gm.mem_pool, stream, db.ptr.value, ds.ptr.value, res.ctypes.data, log_n, ffi.JACOBIAN)
                best = None
                for _ in range(4):
                    ffi.check(lib.panda_msm_execute_bn254(cfg), "msm")
                    phases = (C.c_float * 8)()
                    ffi.check(lib.panda_msm_last_phase_ms(phases), "phases")
                    named = {lib.panda_msm_phase_name(i).decode(): phases[i] for i in range(8) if lib.panda_msm_phase_name(i)}
                    acc = [v for k, v in named.items() if "accum" in k and v > 0]
                    if acc and (best is None or acc[0] < best):
                        best = acc[0]
                ffi.check(lib.panda_msm_set_phase_timing(0), "timing")
                ffi.check(lib.panda_msm_unregister_bases(db.ptr), "unregister")
                if best:
                    emit({"what": "k_accumulate", "curve": "bn254", "log_n": log_n, "tables": tables.value, "window_bits": bits.value, "accumulate_ms": round(best, 4),
                          "additions_per_s": round(n * tables.value / best * 1e3)})
            finally:
                db.free()
                ds.free()
        for curve in curves:
            for log_n in (16, 20):
                n = 1 << log_n
                triple, point = POINT[curve] * 3 // 2, POINT[curve]
                bases, scal = po.gen_bases(curve, 0xAF, 64), po.gen_scalars(po.FR_OF[curve], 0xAE, 64)
                one = pgm.panda_msm_bn254_gpu(gm, scal, bases, curve).view(np.uint8)
                src, dst, cs, cd = DeviceBuffer(n * triple), DeviceBuffer(n * point), DeviceBuffer((triple + point) * n // 2), DeviceBuffer((triple + point) * n // 2)
                try:
                    host = np.tile(one, n)
                    ffi.check(lib.panda_memcpy(src.ptr, C.c_void_p(host.ctypes.data), host.nbytes), "memcpy")

                    def convert():
                        ffi.check(lib.panda_points_to_affine(curve, src.ptr, ffi.JACOBIAN, dst.ptr, n, stream), "to_affine")

                    def copy():
                        ffi.check(lib.panda_memcpy(cd.ptr, cs.ptr, (triple + point) * n // 2), "copy")
                        ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")

                    convert()
                    got = dst.to_host(np.uint8).reshape(n, point)
                    if not (got == got[0]).all() or not got[0].any():
                        raise SystemExit("to_affine: equal triples gave different points")
                    ms = alternate({"M": copy, "A": convert, "m": copy}, "MAm", max(a.alternations, 5))
                    med = {k: statistics.median(v) for k, v in ms.items()}
                    emit({"what": "points_to_affine", "curve": NAME[curve], "log_n": log_n, "traffic_bytes": (triple + point) * n,
                          "median_ms": {k: round(v, 4) for k, v in med.items()}, "to_copy": round(med["A"] / med["M"], 2)})
                finally:
                    for b in (src, dst, cs, cd):
                        b.free()
        if a.once:
            log_n, n = a.once, 1 << a.once
            bufs = [DeviceBuffer(n * 64)]
            try:
                ffi.check(lib.panda_gen_bases(0, 0xEC, 0, n, bufs[0].ptr, NULL_STREAM), "gen")
                ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")
                t0 = time.perf_counter()
                transform(0, bufs[0], bufs[0], log_n, 1)
                emit({"what": "ec_ntt_once", "curve": "bn254", "log_n": log_n, "direction": "inverse, in place", "ms": round((time.perf_counter() - t0) * 1e3, 2)})
            finally:
                bufs[0].free()
        lines = ["what              curve      log_n | forward ms  inverse ms | Gops/s F   Gops/s I"]
        for r in recs:
            if r["what"] == "ec_ntt":
                lines.append("%-17s %-10s %5d | %10.3f  %10.3f | %8.2f  %8.2f" % ("ec_ntt", r["curve"], r["log_n"], r["median_ms"]["F"], r["median_ms"]["I"],
                                                                                r["group_ops_per_s"]["F"] / 1e9, r["group_ops_per_s"]["I"] / 1e9))
        text = "\n".join(lines)
        print(text, flush=True)
        if out_file:
            out_file.write(text + "\n")
    finally:
        if out_file:
            out_file.close()
        gm.deinit()


if __name__ == "__main__":
    main()
