"""The measurement the Poseidon calls stand on (panda_poseidon_permute / _hash / _merkle_tree).  Nobody has measured this before, so
there is no bar; the expectation written next to every result is arithmetic: a BN254 circomlib permutation at t = 3 is 243 Montgomery and
585 Shoup products, 828 in all, and at the ~150 G products/s of profiles/r03_ubench_shoup.txt that is 828 / 150e9 = 5.5 ns.  Other shapes
are scaled by their product counts.  Arms:
  P  panda_poseidon_permute in place at 2^20 states, t = 3 and t = 5, BN254 Fr (circomlib's sets) and BLS12-381 Fr (the paper's generator
     at the same round numbers): ns per permutation, permutations per second, measured / expected;
  1  one permutation (n = 1): launch, one dependent chain of R_F + R_P rounds, synchronise -- the latency unit of the tree's top levels;
  T  panda_poseidon_merkle_tree at heights 10, 16, 20, 24 (arity 2) and 5, 8, 10 (arity 4): ms per tree, ns per node, and the share of the
     call that is NOT throughput work, 1 - nodes x (ns per permutation of arm P) / time: launches, the chain of the top levels, the
     synchronise;
  H  panda_poseidon_hash of 2^20 messages of 8 elements, contiguous rows against the column layout of the batched transforms.
Before anything is timed the outputs are checked against a second route: every tree's root against panda_poseidon_hash run level by
level over the same leaves, the two layouts of arm H against each other, and the first states of arm P against tests/poseidon_ref.py.
Wall clock around calls that end in the library's own synchronise; the arms of a group are alternated --alternations times, each timed
over enough calls to last --min-seconds; medians.  One JSON line per arm, then a table.

usage: poseidon_bench.py [--alternations N] [--min-seconds S] [--out FILE] [--max-height H]"""
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

FIELD = ("BN254 Fr", "BLS12-377 Fr", "BLS12-381 Fr")
PRODUCTS_PER_SECOND = 150e9  # profiles/r03_ubench_shoup.txt
SBOX_PRODUCTS = {5: 3, 7: 4, 11: 5, 17: 5}


def products(P):
    """(Montgomery, Shoup) products of one permutation"""
    return SBOX_PRODUCTS[P.alpha] * (P.rf * P.t + P.rp), (P.rf + P.rp) * P.t * P.t


def expected_ns(P):
    return sum(products(P)) / PRODUCTS_PER_SECOND * 1e9


def device_name():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return f"{p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs)"
    except Exception as e:  # noqa: BLE001
        return f"unknown ({type(e).__name__})"


def alternate(arms, alternations, min_seconds):
    """arms: {name: callable} -> {name: median ms per call}, every arm warmed up, the arms alternated"""
    reps = {}
    for name, run in arms.items():
        run()
        t0 = time.perf_counter()
        run()
        reps[name] = max(1, int(min_seconds / max(time.perf_counter() - t0, 1e-6)) + 1)
    ms = {name: [] for name in arms}
    for _ in range(alternations):
        for name, run in arms.items():
            t0 = time.perf_counter()
            for _ in range(reps[name]):
                run()
            ms[name].append((time.perf_counter() - t0) / reps[name] * 1e3)
    return {name: statistics.median(v) for name, v in ms.items()}, {name: max(v) - min(v) for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.1)
    ap.add_argument("--max-height", type=int, default=24)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import field_ref as fr
    import poseidon_ref as pr
    from gpu_util import NULL_STREAM, DeviceBuffer
    from panda_amd import gpu_manager as pgm
    lib = ffi.load()
    gm = pgm.PandaGpuManager(0)
    stream = gm.exec_stream.raw
    out = open(a.out, "a") if a.out else None
    name = device_name()
    lines = []

    def emit(rec):
        rec["device"] = name
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def handle_of(P):
        rc_w, mds_w = P.rc_wire(), P.mds_wire()
        params = ffi.PoseidonParams(P.t, P.alpha, P.rf, P.rp, rc_w.ctypes.data, mds_w.ctypes.data)
        h = ffi.PandaPoseidon()
        ffi.check(lib.panda_poseidon_create(P.field, C.byref(params), C.byref(h)), "create")
        return h

    def random_elements(field, seed, count):
        d = DeviceBuffer(count * 32)
        ffi.check(lib.panda_gen_scalars(field, seed, 0, count, d.ptr, NULL_STREAM), "gen")
        ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")
        return d

    sets = {(0, 3): pr.circomlib(3), (0, 5): pr.circomlib(5), (2, 3): pr.grain_params(2, 3, 8, 57), (2, 5): pr.grain_params(2, 5, 8, 60)}
    handles = {key: handle_of(P) for key, P in sets.items()}
    bufs = []
    try:
        # ---- arm P and arm 1
        n = 1 << 20
        arms, state_bufs = {}, {}
        for (field, t), P in sets.items():
            d = random_elements(field, 0xB0 + t, n * t)
            bufs.append(d)
            first = d.to_host(np.uint32, nbytes=4 * t * 32).reshape(4, t, 8)
            ffi.check(lib.panda_poseidon_permute(handles[field, t], d.ptr, d.ptr, n, stream), "permute")
            got = d.to_host(np.uint32, nbytes=4 * t * 32).reshape(4, t, 8)
            want = [pr.permute(P, fr.plain(field, s)) for s in first]
            if not np.array_equal(got.reshape(-1, 8), fr.wire(field, [v for s in want for v in s])):
                raise SystemExit(f"field {field} t {t}: the permutation differs from the reference")
            state_bufs[field, t] = d
            arms["P %d %d" % (field, t)] = lambda h=handles[field, t], d=d: ffi.check(lib.panda_poseidon_permute(h, d.ptr, d.ptr, n, stream), "permute")
        one = state_bufs[0, 3]
        arms["1"] = lambda: ffi.check(lib.panda_poseidon_permute(handles[0, 3], one.ptr, one.ptr, 1, stream), "permute")
        med, spread = alternate(arms, a.alternations, a.min_seconds)
        per_perm_ns = {}
        for (field, t), P in sets.items():
            ms = med["P %d %d" % (field, t)]
            ns = ms * 1e6 / n
            per_perm_ns[field, t] = ns
            mont, shoup = products(P)
            emit({"arm": "permute", "field": field, "width": t, "n": n, "median_ms": round(ms, 5), "spread_ms": round(spread["P %d %d" % (field, t)], 5),
                  "ns_per_permutation": round(ns, 3), "permutations_per_s": round(1e9 / ns), "products": [mont, shoup],
                  "expected_ns": round(expected_ns(P), 3), "measured_over_expected": round(ns / expected_ns(P), 3),
                  "products_per_s": round((mont + shoup) / ns * 1e9)})
            lines.append("permute   %-13s t = %d  2^20 states   %9.4f ms   %7.2f ns / permutation   %6.1f M / s   %d + %d products   expected %5.2f ns   measured / expected %5.2f"
                         % (FIELD[field], t, ms, ns, 1e3 / ns, mont, shoup, expected_ns(P), ns / expected_ns(P)))
        emit({"arm": "one permutation", "field": 0, "width": 3, "median_ms": round(med["1"], 5), "spread_ms": round(spread["1"], 5)})
        lines.append("one permutation (BN254, t = 3, launch + chain + synchronise)   %9.4f ms" % med["1"])

        # ---- arm T
        arms, shapes, keep = {}, [], []
        for t, heights in ((3, (10, 16, 20, 24)), (5, (5, 8, 10))):
            a_ = t - 1
            for height in heights:
                if a_ ** height > 2 ** a.max_height:
                    continue
                leaves_n = a_ ** height
                nodes_n, top, launches = C.c_uint64(0), C.c_uint(0), C.c_uint(0)
                offsets = (C.c_uint64 * height)()
                ffi.check(lib.panda_poseidon_plan(t, height, None, C.byref(nodes_n), offsets, C.byref(top), C.byref(launches)), "plan")
                leaves = random_elements(0, 0xC0 + height, leaves_n)
                nodes, alt = DeviceBuffer(nodes_n.value * 32), DeviceBuffer(nodes_n.value * 32)
                bufs += [leaves, nodes, alt]
                tag = fr.wire_one(0, 0x7A6)
                tp = C.c_void_p(tag.ctypes.data)
                root = np.zeros(8, np.uint32)
                h = handles[0, t]
                ffi.check(lib.panda_poseidon_merkle_tree(h, leaves.ptr, height, tp, nodes.ptr, C.c_void_p(root.ctypes.data), stream), "tree")
                below, count = leaves.ptr, leaves_n
                for l in range(1, height + 1):  # the second route: the sponge over each level
                    count //= a_
                    level = C.c_void_p(alt.ptr.value + offsets[l - 1] * 32)
                    ffi.check(lib.panda_poseidon_hash(h, below, a_, a_, 1, tp, level, count, stream), "hash")
                    below = level
                if not np.array_equal(alt.to_host(np.uint32, nbytes=32, offset=(nodes_n.value - 1) * 32), root) or not root.any():
                    raise SystemExit(f"tree t {t} height {height}: the root differs from the hash over each level")
                shapes.append((t, height, nodes_n.value, top.value, launches.value))
                arms["T %d %d" % (t, height)] = (lambda h=h, leaves=leaves, height=height, tp=tp, nodes=nodes:
                                                 ffi.check(lib.panda_poseidon_merkle_tree(h, leaves.ptr, height, tp, nodes.ptr, None, stream), "tree"))
                keep.append(tag)  # the tag's bytes outlive the loop
        med, spread = alternate(arms, a.alternations, a.min_seconds)
        for t, height, nodes_n, top, launches in shapes:
            ms = med["T %d %d" % (t, height)]
            work_ms = nodes_n * per_perm_ns[0, t] / 1e6
            emit({"arm": "merkle_tree", "field": 0, "width": t, "arity": t - 1, "height": height, "nodes": nodes_n, "top_levels": top, "launches": launches,
                  "median_ms": round(ms, 5), "spread_ms": round(spread["T %d %d" % (t, height)], 5), "ns_per_node": round(ms * 1e6 / nodes_n, 3),
                  "throughput_work_ms": round(work_ms, 5), "latency_share": round(max(0.0, 1 - work_ms / ms), 4)})
            lines.append("tree      arity %d  height %2d  %9d nodes  %2d launches (%d top levels)   %10.4f ms   %9.2f ns / node   throughput work %9.4f ms   launch + chain share %5.1f %%"
                         % (t - 1, height, nodes_n, launches, top, ms, ms * 1e6 / nodes_n, work_ms, 100 * max(0.0, 1 - work_ms / ms)))

        # ---- arm H
        n, length = 1 << 20, 8
        src = random_elements(0, 0xD0, n * length)
        ha, hb = DeviceBuffer(n * 32), DeviceBuffer(n * 32)
        bufs += [src, ha, hb]
        tag = fr.wire_one(0, 8)
        tp = C.c_void_p(tag.ctypes.data)
        h = handles[0, 3]
        # the same buffer read as rows and as columns holds different messages: transpose a sample on the host for the cross-check
        sample = src.to_host(np.uint32, nbytes=64 * length * 32).reshape(64, length, 8)
        cols = DeviceBuffer.from_host(np.ascontiguousarray(sample.transpose(1, 0, 2)))
        bufs.append(cols)
        ffi.check(lib.panda_poseidon_hash(h, src.ptr, length, length, 1, tp, ha.ptr, 64, stream), "hash")
        ffi.check(lib.panda_poseidon_hash(h, cols.ptr, length, 1, 64, tp, hb.ptr, 64, stream), "hash")
        rows = ha.to_host(np.uint32, nbytes=64 * 32)
        if not np.array_equal(rows, hb.to_host(np.uint32, nbytes=64 * 32)):
            raise SystemExit("hash: the column layout differs from the contiguous one")
        if not np.array_equal(rows.reshape(-1, 8)[:4], fr.wire(0, [pr.hash(sets[0, 3], fr.plain(0, m), 8) for m in sample[:4]])):
            raise SystemExit("hash: differs from the reference")
        arms = {"H rows": lambda: ffi.check(lib.panda_poseidon_hash(h, src.ptr, length, length, 1, tp, ha.ptr, n, stream), "hash"),
                "H columns": lambda: ffi.check(lib.panda_poseidon_hash(h, src.ptr, length, 1, n, tp, hb.ptr, n, stream), "hash")}
        med, spread = alternate(arms, a.alternations, a.min_seconds)
        chunks = -(-length // 2)
        for layout in ("rows", "columns"):
            ms = med["H " + layout]
            emit({"arm": "hash", "layout": layout, "field": 0, "width": 3, "n": n, "len": length, "median_ms": round(ms, 5), "spread_ms": round(spread["H " + layout], 5),
                  "ns_per_permutation": round(ms * 1e6 / (n * chunks), 3)})
            lines.append("hash      2^20 x %d, t = 3, %-8s   %9.4f ms   %7.2f ns / permutation (%d per message)" % (length, layout, ms, ms * 1e6 / (n * chunks), chunks))
        lines.append("hash      columns / rows   %.3f" % (med["H columns"] / med["H rows"]))
        text = "\n".join(lines)
        print(text, flush=True)
        if out:
            out.write(text + "\n")
    finally:
        for d in bufs:
            d.free()
        for h in handles.values():
            lib.panda_poseidon_destroy(h)
        if out:
            out.close()
        gm.deinit()


if __name__ == "__main__":
    main()
