"""The measurement panda_ntt_execute_lde stands on: `batch` polynomials of 2^log_n coefficients to the coset g H_N of the 2^log_blowup
times larger domain, coefficients resident in a device buffer of their own, as
  arm Z: today's route -- panda_memset_async (hipMemsetAsync) of the batch x N buffer, `batch` strided device copies of the coefficients
         into it, panda_ntt_execute_batch(COSET) at log2 N -- existing entry points only, so it is what a caller has without this call;
  arm C: ONE panda_ntt_execute_lde, COSET_MAJOR order;
  arm N: ONE panda_ntt_execute_lde, NATURAL order (one more streaming kernel);
  arm z: arm Z again (the A/A of the baseline: its run-to-run spread in the same alternation).
One process, the arms share their buffers, outputs compared byte for byte before anything is timed (N against Z directly, C through the
permutation), every shape warmed up (tables cached), wall clock around calls that end in the library's own synchronise, the arms alternated
Z, C, N, z --alternations times, each arm timed over enough calls to last --min-seconds.  Milliseconds per call.  One JSON line per
configuration, then a table with the verdicts of DESIGN.md 5.2.

usage: lde_bench.py [--configs field:log_n:log_blowup:batch,...] [--alternations N] [--min-seconds S] [--out FILE] [--no-verify]"""
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

DEFAULT_CONFIGS = "0:16:3:16,0:18:2:8,0:20:3:4,0:22:2:1"
COSET_ENTRY = ("panda_ntt_execute_bn254_coset", "panda_ntt_execute_bls12_377_coset", "panda_ntt_execute_bls12_381_coset")
FIELD = ("BN254 Fr", "BLS12-377 Fr", "BLS12-381 Fr")
ARMS = "ZCNz"
SHIFT = 5


def device_line(lib, run):
    """device name and the shader clock one call ran at (panda_set_clock_stamps, as bench.py records it)"""
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        name = f"{p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs)"
    except Exception as e:  # noqa: BLE001
        name = f"unknown ({type(e).__name__})"
    mhz = None
    lib.panda_set_clock_stamps(1)
    clk = (C.c_uint64 * ffi.CLOCK_WORDS)()
    run()
    lib.panda_ntt_last_clock(clk)
    lib.panda_set_clock_stamps(0)
    if clk[1]:
        mhz = round(int(clk[3]) / int(clk[1]) * 100.0)
    return name, mhz


def passes_of(lib, log_n):
    p = C.c_uint(0)
    ffi.check(lib.panda_ntt_pass_plan(log_n, C.byref(p), None), "plan")
    return p.value


def table(recs):
    lines = ["field         shape (n x B, polys)   passes Z -> LDE | Z zero-pad route (ms/call)    | z = Z again (A/A)             | C COSET_MAJOR                 | N NATURAL                     | C/Z     N/Z     passes' ms Z / C  sclk MHz"]
    fmt = lambda v: "%8.4f /%8.4f /%8.4f" % tuple(v)
    for r in recs:
        lines.append("%-13s 2^%-2d x %-2d, %-3d          %d -> %d          | %s | %s | %s | %s | %.4f  %.4f  %8.4f / %8.4f  %s" % (
            FIELD[r["field"]], r["log_n"], 1 << r["log_blowup"], r["batch"], r["passes_padded"], r["passes_lde"], fmt(r["Z_min_med_max"]),
            fmt(r["z_min_med_max"]), fmt(r["C_min_med_max"]), fmt(r["N_min_med_max"]), r["C_over_Z_median"], r["N_over_Z_median"],
            r["passes_device_ms"]["Z"], r["passes_device_ms"]["C"], r["sclk_mhz"]))
    lines.append("")
    lines.append("Verdicts.  spread = the baseline's A/A: the larger of max - min over Z's repetitions, over z's, and |median Z - median z|.")
    for r in recs:
        lines.append("%-13s 2^%-2d x %-2d, %-3d: spread %.4f ms; C median - Z median = %+.4f ms: C is %s; N median - C median = %+.4f ms (the interleave); "
                     "butterfly layers %d / %d = %.3f of the padded transform's, measured passes' device time C / Z = %.3f, whole call C / Z = %.3f" % (
                         FIELD[r["field"]], r["log_n"], 1 << r["log_blowup"], r["batch"], r["baseline_spread_ms"], r["C_minus_Z_median_ms"],
                         "NOT SLOWER than the zero-pad route by more than its spread" if r["C_not_slower_beyond_spread"] else "SLOWER than the zero-pad route by more than its spread",
                         r["N_minus_C_median_ms"], r["log_n"], r["log_n"] + r["log_blowup"], r["log_n"] / (r["log_n"] + r["log_blowup"]),
                         r["passes_device_ms"]["C"] / r["passes_device_ms"]["Z"], r["C_over_Z_median"]))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=DEFAULT_CONFIGS)
    ap.add_argument("--alternations", type=int, default=10)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--out")
    ap.add_argument("--no-verify", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import oracle as po
    import pyref
    from gpu_util import NULL_STREAM, DeviceBuffer
    from panda_amd import gpu_manager as pgm
    lib = ffi.load()
    gm = pgm.PandaGpuManager(0)
    out = open(a.out, "a") if a.out else None
    recs = []
    try:
        for spec in a.configs.split(","):
            field, k, lb, batch = (int(x) for x in spec.split(":"))
            n, big = 1 << k, 1 << (k + lb)
            fid = po.FR_OF[field]
            r = pyref.limbs_to_int(po.field_info(fid)["p"])
            g = np.array(pyref.int_to_limbs(SHIFT * (1 << 256) % r, 8), np.uint32)
            gp = C.c_void_p(g.ctypes.data)
            omega = po.root_of_unity(fid, k + lb)
            om = C.c_void_p(omega.ctypes.data)
            coeffs, src, dst = DeviceBuffer(batch * n * 32), DeviceBuffer(batch * big * 32), DeviceBuffer(batch * big * 32)
            flag = C.c_uint(9)
            try:
                ffi.check(lib.panda_gen_scalars(field, 0x1DE + k, 0, batch * n, coeffs.ptr, NULL_STREAM), "gen")
                ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")
                stream = gm.exec_stream.raw
                cfg_big = ffi.NttconfigurationV1(gm.mem_pool, stream, src.ptr, dst.ptr, om, k + lb, C.pointer(flag))
                cfg_lde = ffi.NttconfigurationV1(gm.mem_pool, stream, src.ptr, dst.ptr, om, k, C.pointer(flag))

                def run_z():
                    ffi.check(lib.panda_memset_async(src.ptr, 0, batch * big * 32, stream), "memset")
                    for p in range(batch):
                        ffi.check(lib.panda_memcpy_async(C.c_void_p(src.ptr.value + p * big * 32), C.c_void_p(coeffs.ptr.value + p * n * 32), n * 32, stream), "copy")
                    ffi.check(lib.panda_ntt_execute_batch(field, ffi.NTT_COSET, cfg_big, batch, gp), "batch")

                def run_c():
                    ffi.check(lib.panda_ntt_execute_lde(field, cfg_lde, coeffs.ptr, lb, batch, gp, ffi.NTT_LDE_COSET_MAJOR), "lde")

                def run_n():
                    ffi.check(lib.panda_ntt_execute_lde(field, cfg_lde, coeffs.ptr, lb, batch, gp, ffi.NTT_LDE_NATURAL), "lde")

                run = {"Z": run_z, "C": run_c, "N": run_n, "z": run_z}
                result = lambda: (dst if flag.value else src).to_host(np.uint32).reshape(batch, big, 8)
                if not a.no_verify:  # the arms' outputs on the same coefficients, byte for byte, before anything is timed
                    run_z()
                    want = result()
                    run_n()
                    if not np.array_equal(result(), want):
                        raise SystemExit(f"field {field} 2^{k} x {1 << lb} x {batch}: NATURAL differs from the zero-pad route")
                    run_c()
                    got = result().reshape(batch, 1 << lb, n, 8).transpose(0, 2, 1, 3).reshape(batch, big, 8)
                    if not np.array_equal(got, want):
                        raise SystemExit(f"field {field} 2^{k} x {1 << lb} x {batch}: COSET_MAJOR differs from the zero-pad route")
                    del want, got
                reps, dev_ms = {}, {arm: [] for arm in ARMS}
                for arm in ARMS:  # warm-up of every shape (tables are cached from here on)
                    run[arm]()
                    t0 = time.perf_counter()
                    run[arm]()
                    reps[arm] = max(1, int(a.min_seconds / max(time.perf_counter() - t0, 1e-6)) + 1)
                name, mhz = device_line(lib, run_c)
                ms = {arm: [] for arm in ARMS}
                last = C.c_float(0)
                for _ in range(a.alternations):
                    for arm in ARMS:
                        t0 = time.perf_counter()
                        for _ in range(reps[arm]):
                            run[arm]()
                        ms[arm].append((time.perf_counter() - t0) / reps[arm] * 1e3)
                        lib.panda_ntt_last_device_ms(C.byref(last))  # the passes of the arm's last call (events around them)
                        dev_ms[arm].append(last.value)
                launches = C.c_uint(0)
                ffi.check(lib.panda_ntt_lde_plan(k, lb, batch, 0, C.byref(launches), None), "plan")
                med = {arm: statistics.median(ms[arm]) for arm in ARMS}
                spread = max(max(ms["Z"]) - min(ms["Z"]), max(ms["z"]) - min(ms["z"]), abs(med["Z"] - med["z"]))
                rec = {"field": field, "log_n": k, "log_blowup": lb, "batch": batch, "passes_padded": passes_of(lib, k + lb), "passes_lde": passes_of(lib, k),
                       "lde_launches_coset_major": launches.value, "device": name, "sclk_mhz": mhz, "calls_per_repetition": reps,
                       "per_call_ms": {arm: [round(v, 5) for v in ms[arm]] for arm in ARMS},
                       "passes_device_ms": {arm: round(statistics.median(dev_ms[arm]), 5) for arm in ARMS}}
                for arm in ARMS:
                    rec[f"{arm}_min_med_max"] = [round(min(ms[arm]), 5), round(med[arm], 5), round(max(ms[arm]), 5)]
                rec["baseline_spread_ms"] = round(spread, 5)
                rec["C_over_Z_median"] = round(med["C"] / med["Z"], 4)
                rec["N_over_Z_median"] = round(med["N"] / med["Z"], 4)
                rec["C_minus_Z_median_ms"] = round(med["C"] - med["Z"], 5)
                rec["N_minus_C_median_ms"] = round(med["N"] - med["C"], 5)
                rec["C_not_slower_beyond_spread"] = med["C"] <= med["Z"] + spread
                recs.append(rec)
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
            finally:
                for d in (coeffs, src, dst):
                    d.free()
        text = table(recs)
        print(text, flush=True)
        if out:
            out.write(text + "\n")
    finally:
        if out:
            out.close()
        gm.deinit()


if __name__ == "__main__":
    main()
