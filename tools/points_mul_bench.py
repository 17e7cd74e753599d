"""The measurement panda_points_scalar_mul and panda_kzg_open_all stand on.  Inputs are panda_gen_bases points and
panda_gen_scalars scalars; nothing is compared with a CPU here (tests/test_points_mul.py and tests/test_kzg_open_all.py do that): before
anything is timed, ONE with s and then with 1 / s must give the points back byte for byte, and at 2^12 proof 1 of an opening set must be
the MSM of the quotient panda_poly_divide_linear forms.  Every call is synchronous (it ends in a synchronise); medians of --reps wall
times, ms per call and ns per point.
  multiplication  2^16 and 2^20 points (--logs) on the curves 0 BN254, 1 BLS12-377, 2 BLS12-381 (--curves): the modes EACH, ONE, POWERS,
                  each with and without an addend; EACH also with scalars below 2^64 and below 2^128 (the loop-length rule: the expected
                  ratio to full length is the ratio of the bit counts, plus the fixed cost of the two launches)
  against         in the same run over the same points: a forward and an inverse panda_ec_ntt of the same size -- their difference is
                  k_scale, one uniform multiplication per point, which ONE is compared with; EACH is compared with the divergent stage of
                  profiles/ec_ntt.txt (a kernel trace of another session) less its two additions
  openings        PandaKzgOpenAll.open at 2^12, 2^16 and 2^20 on BN254 and at 2^16 on the BLS curves (--open-logs, --open-bls-log), the
                  setup call apart; the parts timed alone at the same sizes (scalar transform of 2n, EACH of 2n, inverse EC-NTT of 2n,
                  forward EC-NTT of n); and one panda_poly_divide_linear + one MSM of size n, times n: the O(n^2) route to the same proofs
One JSON line per record, then a table.

usage: points_mul_bench.py [--curves 0,1,2] [--logs 16,20] [--open-logs 12,16,20] [--open-bls-log 16] [--reps N] [--out FILE]"""
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
R = {0: 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001, 1: 0x12AB655E9A2CA55660B44D1E5C37B00159AA76FED00000010A11800000000001,
     2: 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001}
NAME = {0: "bn254", 1: "bls12_377", 2: "bls12_381"}
MODE = {0: "each", 1: "one", 2: "powers"}


def device_name():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return f"{p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs)"
    except Exception as e:  # noqa: BLE001
        return f"unknown ({type(e).__name__})"


def median_ms(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="0,1,2")
    ap.add_argument("--logs", default="16,20")
    ap.add_argument("--open-logs", default="12,16,20")
    ap.add_argument("--open-bls-log", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
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

    def wire(curve, v):
        return np.frombuffer((v % R[curve] * (1 << 256) % R[curve]).to_bytes(32, "little"), np.uint32).copy()

    def hp(x):
        return None if x is None else C.c_void_p(x.ctypes.data)

    def mul(curve, mode, pts, d_sc, h_sc, add, out, n):
        ffi.check(lib.panda_points_scalar_mul(curve, mode, pts.ptr, None if d_sc is None else d_sc.ptr, hp(h_sc), None if add is None else add.ptr, out.ptr, n, stream),
                  "points_scalar_mul")

    def transform(curve, src, dst, log_n, direction):
        om = np.ascontiguousarray(po.root_of_unity(po.FR_OF[curve], log_n))
        ffi.check(lib.panda_ec_ntt(curve, src.ptr, dst.ptr, log_n, direction, hp(om), stream), "ec_ntt")

    def gen(curve, n, seed):
        pts, sc = DeviceBuffer(n * POINT[curve]), DeviceBuffer(n * 32)
        ffi.check(lib.panda_gen_bases(curve, seed, 0, n, pts.ptr, NULL_STREAM), "gen")
        ffi.check(lib.panda_gen_scalars(curve, seed + 1, 0, n, sc.ptr, NULL_STREAM), "gen")
        ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")
        return pts, sc

    def short_scalars(curve, n, bits):
        """n Montgomery-form scalars whose integers are below 2^bits"""
        raw = np.random.default_rng(bits).integers(0, 1 << 32, (n, bits // 32), dtype=np.uint64).astype(np.uint32)
        mont = (1 << 256) % R[curve]
        vals = [int.from_bytes(row.tobytes(), "little") * mont % R[curve] for row in raw]
        return DeviceBuffer.from_host(np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), np.uint32).copy())

    try:
        curves, logs = [int(c) for c in a.curves.split(",")], [int(v) for v in a.logs.split(",")]
        for curve in curves:
            for log_n in logs:
                n = 1 << log_n
                pts, sc = gen(curve, n, 0x9B)
                add, out, back = DeviceBuffer(n * POINT[curve]), DeviceBuffer(n * POINT[curve]), DeviceBuffer(n * POINT[curve])
                extra = []
                try:
                    ffi.check(lib.panda_gen_bases(curve, 0x9D, 0, n, add.ptr, NULL_STREAM), "gen")
                    ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")
                    s = 0x1234567 * R[curve] // 0x7654321
                    mul(curve, 1, pts, None, wire(curve, s), None, out, n)
                    mul(curve, 1, out, None, wire(curve, pow(s, -1, R[curve])), None, back, n)
                    if not np.array_equal(pts.to_host(), back.to_host()):
                        raise SystemExit(f"curve {curve} 2^{log_n}: ONE with s, then with 1 / s, does not return the points")
                    host = {1: wire(curve, s), 2: np.concatenate([wire(curve, 3), wire(curve, s)])}
                    rec = {"what": "points_scalar_mul", "curve": NAME[curve], "log_n": log_n, "ms": {}, "ns_per_point": {}}
                    for mode in (0, 1, 2):
                        for with_add in (False, True):
                            ms = median_ms(lambda: mul(curve, mode, pts, sc if mode == 0 else None, host.get(mode), add if with_add else None, out, n), a.reps)
                            key = MODE[mode] + ("+a" if with_add else "")
                            rec["ms"][key], rec["ns_per_point"][key] = round(ms, 4), round(ms * 1e6 / n, 2)
                    for bits in (64, 128):
                        short = short_scalars(curve, n, bits)
                        extra.append(short)
                        ms = median_ms(lambda: mul(curve, 0, pts, short, None, None, out, n), a.reps)
                        rec["ms"]["each<2^%d" % bits], rec["ns_per_point"]["each<2^%d" % bits] = round(ms, 4), round(ms * 1e6 / n, 2)
                    f_ms = median_ms(lambda: transform(curve, pts, out, log_n, 0), a.reps)
                    i_ms = median_ms(lambda: transform(curve, pts, out, log_n, 1), a.reps)
                    rec["ec_ntt_forward_ms"], rec["ec_ntt_inverse_ms"] = round(f_ms, 4), round(i_ms, 4)
                    rec["k_scale_ns_per_point"] = round((i_ms - f_ms) * 1e6 / n, 2)
                    emit(rec)
                finally:
                    for b in [pts, sc, add, out, back] + extra:
                        b.free()

        def opening(curve, log_n):
            n = 1 << log_n
            srs, coeffs = gen(curve, n, 0x9F)
            om2 = np.ascontiguousarray(po.root_of_unity(po.FR_OF[curve], log_n + 1))
            h_srs, h_coeffs = srs.to_host(np.uint8), coeffs.to_host(np.uint32).reshape(n, 8)
            t0 = time.perf_counter()
            opener = pgm.PandaKzgOpenAll(gm, h_srs, om2, curve)  # stages the SRS and runs the setup call
            setup_ms = (time.perf_counter() - t0) * 1e3
            big, sc2 = gen(curve, 2 * n, 0xA1)
            work = DeviceBuffer(2 * n * 32)
            quot, res = DeviceBuffer(n * 32), np.zeros(POINT[curve] * 3 // 8, np.uint32)
            try:
                def open_device():
                    ffi.check(lib.panda_kzg_open_all(curve, coeffs.ptr, opener.d_table, log_n, hp(om2), opener.d_work, opener.work_bytes, opener.d_proofs, stream), "open")

                open_ms = median_ms(open_device, a.reps)
                proofs = opener.open(h_coeffs)
                # the O(n^2) route: one division and one MSM of size n, and proof 1 both ways
                w = (lambda v: v * v % R[curve])(int.from_bytes(om2.tobytes(), "little") * pow(1 << 256, -1, R[curve]) % R[curve])
                z = wire(curve, w)
                cfg = ffi.MSMConfiguration(gm.mem_pool, stream, srs.ptr.value, quot.ptr.value, res.ctypes.data, log_n, ffi.JACOBIAN)
                msm = [lib.panda_msm_execute_bn254, lib.panda_msm_execute_bls12_377, lib.panda_msm_execute_bls12_381][curve]

                def one_proof():
                    ffi.check(lib.panda_poly_divide_linear(curve, coeffs.ptr, quot.ptr, n, 1, hp(z), None, stream), "divide")
                    ffi.check(msm(cfg), "msm")

                one_ms = median_ms(one_proof, max(a.reps, 5))
                if log_n <= 12:
                    import pyref
                    c = pyref.CURVES[curve]
                    if pyref.decode_jacobian(c, res) != pyref.decode_affine(c, proofs[1].view(np.uint32)):
                        raise SystemExit(f"curve {curve} 2^{log_n}: proof 1 is not the MSM of the quotient")
                # the parts alone, at the sizes the composite runs them
                flag = C.c_uint(0)
                ncfg = ffi.NttconfigurationV1(gm.mem_pool, stream, sc2.ptr.value, work.ptr.value, om2.ctypes.data, log_n + 1, C.pointer(flag))
                parts = {"scalar_ntt_2n": median_ms(lambda: ffi.check(lib.panda_ntt_execute_batch(curve, ffi.NTT_FORWARD, ncfg, 1, None), "ntt"), a.reps),
                         "each_2n": median_ms(lambda: mul(curve, 0, big, sc2, None, None, big, 2 * n), a.reps),
                         "ec_ntt_inverse_2n": median_ms(lambda: transform(curve, big, big, log_n + 1, 1), a.reps),
                         "ec_ntt_forward_n": median_ms(lambda: transform(curve, srs, srs, log_n, 0), a.reps)}
                emit({"what": "kzg_open_all", "curve": NAME[curve], "log_n": log_n, "open_ms": round(open_ms, 3), "setup_with_staging_ms": round(setup_ms, 3),
                      "parts_ms": {k: round(v, 3) for k, v in parts.items()}, "parts_sum_ms": round(sum(parts.values()), 3),
                      "divide_plus_msm_ms": round(one_ms, 4), "n_times_divide_plus_msm_s": round(one_ms * n / 1e3, 2),
                      "speedup": round(one_ms * n / open_ms, 1)})
            finally:
                opener.close()
                for b in (srs, coeffs, big, sc2, work, quot):
                    b.free()

        for log_n in [int(v) for v in a.open_logs.split(",") if v]:
            if 0 in curves:
                opening(0, log_n)
        for curve in curves:
            if curve and a.open_bls_log:
                opening(curve, a.open_bls_log)

        lines = ["points_scalar_mul, ns per point", "curve      log_n |    each  each+a     one   one+a  powers powers+a | each<2^64 each<2^128 | k_scale (I - F)"]
        for r in recs:
            if r["what"] == "points_scalar_mul":
                p = r["ns_per_point"]
                lines.append("%-10s %5d | %7.2f %7.2f %7.2f %7.2f %7.2f %8.2f | %9.2f %10.2f | %8.2f" % (
                    r["curve"], r["log_n"], p["each"], p["each+a"], p["one"], p["one+a"], p["powers"], p["powers+a"], p["each<2^64"], p["each<2^128"], r["k_scale_ns_per_point"]))
        lines += ["kzg_open_all, ms", "curve      log_n |     open  parts sum | scalar ntt  each 2n  inverse 2n  forward n | setup+staging | divide+msm  x n, s  speedup"]
        for r in recs:
            if r["what"] == "kzg_open_all":
                p = r["parts_ms"]
                lines.append("%-10s %5d | %8.2f %10.2f | %10.3f %8.2f %11.2f %10.2f | %13.2f | %10.4f %7.2f %8.1f" % (
                    r["curve"], r["log_n"], r["open_ms"], r["parts_sum_ms"], p["scalar_ntt_2n"], p["each_2n"], p["ec_ntt_inverse_2n"], p["ec_ntt_forward_n"],
                    r["setup_with_staging_ms"], r["divide_plus_msm_ms"], r["n_times_divide_plus_msm_s"], r["speedup"]))
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
