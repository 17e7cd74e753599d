"""Index-level model of the three launches of panda_field_batch_inverse / panda_poly_grand_product (csrc/poly_product.hip): the thread ->
element maps (E consecutive elements per thread, WAVE lanes, WAVES waves, tile = E * WAVE * WAVES), the cross-lane product scans in either
direction, the combination of the waves, the seed kernel's three walks over chunks of THREADS * CE tile totals (grand denominator product
and its ONE inverse; suffix seeds from the last chunk down; prefix seeds from the first chunk up, both replacing the totals), and the apply
launch with its workgroups run one after the other in an arbitrary order on an output that may be one of the inputs.  Exact integers
modulo a 31-bit prime (products fit 64 bits, so numpy carries a workgroup's threads at once); elements beyond n read as one and stores
beyond n are dropped, as in the kernels.  The radix constant of the kernels' arithmetic is not modelled: residues are plain.  Checked
against the plain definitions (pow(x, -1, P), running products).  Development aid; tests/test_poly_product.py runs it on the CPU with the
tile and carry chunk panda_poly_product_plan reports.

usage: model_poly_product.py            (self-check: small shapes exhaustively, the library's shape at its boundary sizes)"""
import numpy as np

P = 2013265921  # 15 * 2^27 + 1
WAVE, WAVES, E, CE = 64, 4, 4, 4  # csrc/poly_product.hip
INVERSE, PRODUCT, RUNNING = 0, 1, 2


class Shape:
    def __init__(self, e=E, wave=WAVE, waves=WAVES, ce=CE):
        assert wave & (wave - 1) == 0 and wave > 1
        self.e, self.wave, self.waves, self.ce = e, wave, waves, ce
        self.threads = wave * waves
        self.tile, self.chunk = e * self.threads, ce * self.threads
        self.log_wave = wave.bit_length() - 1

    @classmethod
    def from_plan(cls, tile, carry_chunk, wave=WAVE, waves=WAVES):
        threads = wave * waves
        assert tile % threads == 0 and carry_chunk % threads == 0
        return cls(tile // threads, wave, waves, carry_chunk // threads)


def inverse_reference(x):
    return np.array([pow(int(v), -1, P) if v else 0 for v in x], np.int64)


def product_reference(num, den):
    """(Z, total) by the plain recurrence; all zero when a denominator is zero"""
    n = len(num)
    if den is not None and not np.all(den):
        return np.zeros(n, np.int64), 0
    z, acc = np.zeros(n, np.int64), 1
    for i in range(n):
        z[i] = acc
        acc = acc * int(num[i]) % P * (pow(int(den[i]), -1, P) if den is not None else 1) % P
    return z, acc


def wave_scan(v, sh, rev):
    """inclusive product scan of every wave (rows): lane l <- prod_{u <= l} v_u (rev: u >= l); lanes without a neighbour keep their value"""
    v = v.copy()
    for s in range(sh.log_wave):
        d = 1 << s
        t = np.ones_like(v)
        if rev:
            t[:, :-d] = v[:, d:]
        else:
            t[:, d:] = v[:, :-d]
        v = v * t % P
    return v


def block_scan(sh, g, seed, rev):
    """block_scan of csrc/poly_scan.h with the product: g (threads,) -> (seed times the g of every thread before (rev: behind) each thread, seed times all)"""
    v = wave_scan(g.reshape(sh.waves, sh.wave), sh, rev)
    wave_total = v[:, 0] if rev else v[:, -1]
    base = np.zeros(sh.waves, np.int64)
    y = seed
    order = range(sh.waves - 1, -1, -1) if rev else range(sh.waves)
    for w in order:
        base[w] = y
        y = y * int(wave_total[w]) % P
    ex = np.ones_like(v)
    if rev:
        ex[:, :-1] = v[:, 1:]
    else:
        ex[:, 1:] = v[:, :-1]
    return (base[:, None] * ex % P).reshape(-1), y


def load_runs(buf, first, count, threads, run, fill=None):
    """`threads` runs of `run` consecutive elements from buf[first ...] (or `fill` for each), one from `count` on"""
    x = np.ones(threads * run, np.int64)
    have = max(0, min(count - first, threads * run))
    x[:have] = buf[first:first + have] if fill is None else fill
    return x.reshape(threads, run)


def run_product(x):
    g = x[:, 0].copy()
    for e in range(1, x.shape[1]):
        g = g * x[:, e] % P
    return g


def block_product(sh, g):
    v = wave_scan(g.reshape(sh.waves, sh.wave), sh, False)[:, -1]
    y = int(v[0])
    for w in range(1, sh.waves):
        y = y * int(v[w]) % P
    return y


def mask_zeros(x):
    z = x == 0
    return np.where(z, 1, x), z


def tile_totals(sh, mode, num, den):
    """launch 1 -> (tn, td); td is untouched (-1) for the inverse"""
    n = len(num)
    tiles = -(-n // sh.tile)
    tn, td = np.full(tiles, -1, np.int64), np.full(tiles, -1, np.int64)
    for a in range(tiles):
        x = load_runs(num, a * sh.tile, n, sh.threads, sh.e)
        if mode == INVERSE:
            x, _ = mask_zeros(x)
        tn[a] = block_product(sh, run_product(x))
        if mode != INVERSE:
            d = load_runs(den, a * sh.tile, n, sh.threads, sh.e, fill=1 if mode == RUNNING else None)
            td[a] = block_product(sh, run_product(d))
    return tn, td


def seeds(sh, mode, tn, td):
    """launch 2, in place on tn and td; returns the vector's total (None for the inverse)"""
    tiles = len(tn)
    chunks = -(-tiles // sh.chunk)
    din = tn if mode == INVERSE else td
    carry = 1
    for k in range(chunks):
        x = load_runs(din, k * sh.chunk, tiles, sh.threads, sh.ce)
        _, carry = block_scan(sh, run_product(x), carry, False)
    inv = pow(carry, P - 2, P)  # zero for zero
    carry = inv
    for k in range(chunks - 1, -1, -1):
        x = load_runs(din, k * sh.chunk, tiles, sh.threads, sh.ce)
        s, carry = block_scan(sh, run_product(x), carry, True)
        out = np.zeros((sh.threads, sh.ce), np.int64)
        for e in range(sh.ce - 1, -1, -1):
            out[:, e] = s
            if e > 0:
                s = s * x[:, e] % P
        have = min(tiles - k * sh.chunk, sh.chunk)
        td[k * sh.chunk:k * sh.chunk + have] = out.reshape(-1)[:have]
    carry = 1
    for k in range(chunks):
        x = load_runs(tn, k * sh.chunk, tiles, sh.threads, sh.ce)
        s, carry = block_scan(sh, run_product(x), carry, False)
        out = np.zeros((sh.threads, sh.ce), np.int64)
        for e in range(sh.ce):
            out[:, e] = s
            if e < sh.ce - 1:
                s = s * x[:, e] % P
        have = min(tiles - k * sh.chunk, sh.chunk)
        tn[k * sh.chunk:k * sh.chunk + have] = out.reshape(-1)[:have]
    return None if mode == INVERSE else carry * inv % P


def apply(sh, mode, num, den, out, sn, sd, order):
    """launch 3: workgroup after workgroup in `order`; out may be num or den itself"""
    n = len(num)
    for a in order:
        x = load_runs(num, a * sh.tile, n, sh.threads, sh.e)  # every thread loads its own indices before it stores them
        if mode == INVERSE:
            x, zeros = mask_zeros(x)
            d = x.copy()
        else:
            d = load_runs(den, a * sh.tile, n, sh.threads, sh.e, fill=1 if mode == RUNNING else None)
        pre, _ = block_scan(sh, run_product(x), int(sn[a]), False)
        suf, _ = block_scan(sh, run_product(d), int(sd[a]), True)
        pref = np.zeros((sh.threads, sh.e), np.int64)
        for e in range(sh.e):
            pref[:, e] = pre
            if e < sh.e - 1:
                pre = pre * x[:, e] % P
        res = np.zeros((sh.threads, sh.e), np.int64)
        for e in range(sh.e - 1, -1, -1):
            if mode != INVERSE:
                suf = suf * d[:, e] % P
            res[:, e] = pref[:, e] * suf % P
            if mode == INVERSE:
                res[:, e] = np.where(zeros[:, e], 0, res[:, e])
                if e > 0:
                    suf = suf * d[:, e] % P
        have = min(n - a * sh.tile, sh.tile)
        out[a * sh.tile:a * sh.tile + have] = res.reshape(-1)[:have]


def run(sh, mode, num, den=None, in_place=None, seed=1):
    """(out, total) by the three launches; in_place: None, "num" or "den"; the apply launch's workgroups run in a shuffled order"""
    num = np.array(num, np.int64)
    den = None if den is None else np.array(den, np.int64)
    tn, td = tile_totals(sh, mode, num, den)
    total = seeds(sh, mode, tn, td)
    out = {None: np.full(len(num), -1, np.int64), "num": num, "den": den}[in_place]
    apply(sh, mode, num, den, out, tn, td, np.random.default_rng(seed).permutation(len(tn)))
    return out, total


def is_inverse(x, out):
    """out_i x_i = 1 where x_i != 0 and out_i = 0 where x_i = 0: the complete characterisation"""
    return bool(np.array_equal(out * x % P, (x != 0).astype(np.int64)) and not np.any(out[x == 0]))


def is_product(num, den, out, total):
    """out_0 = 1, out_(i+1) den_i = out_i num_i, total den_(n-1) = out_(n-1) num_(n-1): the complete characterisation when no denominator
    is zero (den None: ones)"""
    den = np.ones_like(num) if den is None else den
    step = out * num % P
    return bool(out[0] == 1 and np.array_equal(out[1:] * den[:-1] % P, step[:-1]) and total * int(den[-1]) % P == int(step[-1]))


def check(sh, n, seed=0, zeros=(), den_zeros=()):
    """all three modes, out of place and in place, against the plain definitions (above 2^16 elements, where the Python loops cost
    seconds: the characterisations, one variant per mode); `zeros` are planted in the inverse's input and the numerators, `den_zeros` in
    the denominators"""
    rng = np.random.default_rng(seed * 1000003 + n)
    x = rng.integers(1, P, n, dtype=np.int64)
    den = rng.integers(1, P, n, dtype=np.int64)
    for i in zeros:
        x[i] = 0
    for i in den_zeros:
        den[i] = 0
    if n > 1 << 16:
        assert not den_zeros
        out, _ = run(sh, INVERSE, x, in_place="num", seed=seed)
        assert is_inverse(x, out), (n, "inverse")
        out, t = run(sh, PRODUCT, x, den, in_place="den", seed=seed)
        assert is_product(x, den, out, t), (n, "product")
        out, t = run(sh, RUNNING, x, seed=seed)
        assert is_product(x, None, out, t), (n, "running")
        return True
    want_inv = inverse_reference(x)
    want_z, want_t = product_reference(x, den)
    want_r, want_rt = product_reference(x, None)
    for in_place in (None, "num"):
        out, _ = run(sh, INVERSE, x, in_place=in_place, seed=seed)
        assert np.array_equal(out, want_inv) and is_inverse(x, out), (n, "inverse", in_place)
        out, t = run(sh, RUNNING, x, in_place=in_place, seed=seed)
        assert np.array_equal(out, want_r) and t == want_rt and is_product(x, None, out, t), (n, "running", in_place)
    for in_place in (None, "num", "den"):
        out, t = run(sh, PRODUCT, x, den, in_place=in_place, seed=seed)
        assert np.array_equal(out, want_z) and t == want_t, (n, "product", in_place)
        assert den_zeros or is_product(x, den, out, t), (n, "product", in_place)
    return True


def boundary_sizes(tile, chunk, e=None, wave=WAVE):
    sizes = [1, 2, 3, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1, 5 * tile - 7, tile * chunk + 1, 2 * tile * chunk + tile + 5]
    if e:
        sizes += [e - 1, e + 1, wave * e - 1, wave * e + 1]
    return sorted({s for s in sizes if s >= 1})


def main():
    small = Shape(e=3, wave=4, waves=2, ce=2)  # tile 24, chunk 16: three carry chunks within a few hundred elements
    for n in range(1, 2 * small.tile * small.chunk + small.tile + 6):
        check(small, n)
    n = small.tile * small.chunk + 1
    for zeros, den_zeros in (((0,), ()), ((n - 1,), ()), (tuple(range(small.tile, 2 * small.tile)), ()), (tuple(range(n)), ()), ((), (0,)), ((), (n // 2,)), ((5,), (n - 1,))):
        check(small, n, zeros=zeros, den_zeros=den_zeros)
    lib = Shape()
    for n in boundary_sizes(lib.tile, lib.chunk, lib.e):
        check(lib, n)
    print("model_poly_product: ok (tile %d, carry chunk %d)" % (lib.tile, lib.chunk))


if __name__ == "__main__":
    main()
