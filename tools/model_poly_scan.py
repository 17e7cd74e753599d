"""Index-level model of the three launches of panda_poly_divide_linear / panda_poly_evaluate (csrc/poly.hip): the thread -> element
maps (E consecutive elements per thread, WAVE lanes, WAVES waves, tile = E * WAVE * WAVES), the cross-lane ladder m^(RUN 2^s), the
combination of the waves, the carry kernel's chunks of THREADS * CE tile totals walked from the last one down and overwritten in place,
and the apply launch with its workgroups run one after the other in an arbitrary order on a buffer that may be the input itself.  Exact
integers modulo a 31-bit prime (products fit 64 bits, so numpy carries a workgroup's threads at once); coefficients beyond n read as
zero and stores beyond n are dropped, as in the kernels.  Checked against plain Horner.  Development aid; tests/test_poly_open.py runs it
on the CPU with the tile and carry chunk panda_poly_plan reports.

usage: model_poly_scan.py            (self-check: small shapes exhaustively, the library's shape at its boundary sizes)"""
import numpy as np

P = 2013265921  # 15 * 2^27 + 1
WAVE, WAVES, E, CE = 64, 4, 8, 4  # csrc/poly.hip


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


def horner_reference(c, z):
    """(q, r): q_j = S_(j+1), r = S_0, by the plain recurrence"""
    n = len(c)
    q = np.zeros(n, np.int64)
    s = 0
    for j in range(n - 1, -1, -1):
        q[j] = s
        s = (int(c[j]) + z * s) % P
    return q, s


def ladder(m, run, log_wave):
    """m^(run 2^s), s = 0 .. log_wave"""
    pw = [pow(m, run, P)]
    for _ in range(log_wave):
        pw.append(pw[-1] * pw[-1] % P)
    return pw


def lanes_up(v, d):
    """value d lanes up within each wave (rows), zero past the wave's end"""
    t = np.zeros_like(v)
    if d < v.shape[1]:
        t[:, :-d] = v[:, d:]
    return t


def wave_steps(v, pw, log_wave):
    """the log_wave cross-lane steps: lane l <- sum_{u >= l} v_u m^(run (u - l)); lane 0 holds the wave's total"""
    for s in range(log_wave):
        v = (v + pw[s] * lanes_up(v, 1 << s)) % P
    return v


def run_horner(x, m):
    """x: (threads, run) -> sum_e x[t][e] m^e"""
    g = x[:, -1].copy()
    for e in range(x.shape[1] - 2, -1, -1):
        g = (x[:, e] + m * g) % P
    return g


def block_suffix_scan(sh, x, edge, m, pw):
    """block_suffix_scan of csrc/poly.hip: x (threads, run) -> (right edge value of every thread, total)"""
    g = run_horner(x, m).reshape(sh.waves, sh.wave)
    totals = wave_steps(g.copy(), pw, sh.log_wave)[:, 0]
    mine = np.zeros(sh.waves, np.int64)
    mine[sh.waves - 1] = edge
    y = edge
    for w in range(sh.waves - 1, -1, -1):
        y = (int(totals[w]) + pw[sh.log_wave] * y) % P
        if w >= 1:
            mine[w - 1] = y
    g[:, sh.wave - 1] = (g[:, sh.wave - 1] + pw[0] * mine) % P
    g = wave_steps(g, pw, sh.log_wave)
    right = lanes_up(g, 1)
    right[:, sh.wave - 1] = mine
    return right.reshape(-1), y


def load_runs(buf, first, count, threads, run):
    """`threads` runs of `run` consecutive elements from buf[first ...], zero from `count` on"""
    x = np.zeros(threads * run, np.int64)
    have = max(0, min(count - first, threads * run))
    x[:have] = buf[first:first + have]
    return x.reshape(threads, run)


def tile_totals(sh, c, z):
    """launch 1"""
    n = len(c)
    tiles = -(-n // sh.tile)
    pw = ladder(z, sh.e, sh.log_wave)
    out = np.zeros(tiles, np.int64)
    for a in range(tiles):
        x = load_runs(c, a * sh.tile, n, sh.threads, sh.e)
        w = wave_steps(run_horner(x, z).reshape(sh.waves, sh.wave), pw, sh.log_wave)[:, 0]
        y = int(w[sh.waves - 1])
        for k in range(sh.waves - 2, -1, -1):
            y = (int(w[k]) + pw[sh.log_wave] * y) % P
        out[a] = y
    return out


def carries(sh, totals, z, store=True):
    """launch 2, in place on `totals` when store is set; returns the value S_0"""
    tiles = len(totals)
    y = pow(z, sh.tile, P)
    pw = ladder(y, sh.ce, sh.log_wave)
    carry = 0
    for k in range(-(-tiles // sh.chunk) - 1, -1, -1):
        x = load_runs(totals, k * sh.chunk, tiles, sh.threads, sh.ce)
        s, carry = block_suffix_scan(sh, x, carry, y, pw)
        if store:
            out = np.zeros((sh.threads, sh.ce), np.int64)
            for e in range(sh.ce - 1, -1, -1):
                out[:, e] = s
                if e > 0:
                    s = (x[:, e] + y * s) % P
            have = min(tiles - k * sh.chunk, sh.chunk)
            totals[k * sh.chunk:k * sh.chunk + have] = out.reshape(-1)[:have]
    return carry


def apply(sh, c, q, carry_of, z, order):
    """launch 3: workgroup after workgroup in `order`; q may be c itself"""
    n = len(c)
    pw = ladder(z, sh.e, sh.log_wave)
    for a in order:
        x = load_runs(c, a * sh.tile, n, sh.threads, sh.e)  # every load of the workgroup precedes its first store
        s, _ = block_suffix_scan(sh, x, int(carry_of[a]), z, pw)
        out = np.zeros((sh.threads, sh.e), np.int64)
        for e in range(sh.e - 1, -1, -1):
            out[:, e] = s
            if e > 0:
                s = (x[:, e] + z * s) % P
        have = min(n - a * sh.tile, sh.tile)
        q[a * sh.tile:a * sh.tile + have] = out.reshape(-1)[:have]


def evaluate(sh, c, z):
    return carries(sh, tile_totals(sh, np.asarray(c, np.int64), z), z, store=False)


def divide(sh, c, z, in_place=False, seed=1):
    """(q, r) by the three launches; the apply launch's workgroups run in a shuffled order"""
    c = np.array(c, np.int64)
    t = tile_totals(sh, c, z)
    r = carries(sh, t, z)
    q = c if in_place else np.full(len(c), -1, np.int64)
    order = np.random.default_rng(seed).permutation(len(t))
    apply(sh, c, q, t, z, order)
    return q, r


def is_quotient(c, z, q, r):
    """q, r are the quotient and remainder of c by X - z if and only if q_(n-1) = 0, q_(j-1) - z q_j = c_j (1 <= j < n) and
    r - z q_0 = c_0: the recurrence read backwards, three vector operations"""
    c, q = np.asarray(c, np.int64), np.asarray(q, np.int64)
    return bool(q[-1] == 0 and np.array_equal((q[:-1] - z * q[1:]) % P, c[1:]) and (r - z * int(q[0])) % P == int(c[0]))


def check(sh, n, seed=0, z=None):
    """the three launches against plain Horner (by the recurrence identity alone above 2^16 elements, where the Python loop costs seconds)"""
    rng = np.random.default_rng(seed * 1000003 + n)
    c = rng.integers(0, P, n, dtype=np.int64)
    z = int(rng.integers(2, P)) if z is None else z
    want = horner_reference(c, z) if n <= 1 << 16 else None
    for in_place in (False, True):
        q, r = divide(sh, c, z, in_place, seed)
        assert is_quotient(c, z, q, r), (n, in_place)
        assert want is None or (r == want[1] and np.array_equal(q, want[0])), (n, in_place)
        assert evaluate(sh, c, z) == r, (n, "evaluate")
    return True


def boundary_sizes(tile, chunk, e=None, wave=WAVE):
    sizes = [1, 2, 3, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1, 5 * tile - 7, tile * chunk + 1, 2 * tile * chunk + tile + 5]
    if e:
        sizes += [e - 1, e + 1, wave * e - 1, wave * e + 1]
    return sorted({s for s in sizes if s >= 1})


def main():
    small = Shape(e=3, wave=4, waves=2, ce=2)  # tile 24, chunk 16: three levels within a few hundred elements
    for n in range(1, 2 * small.tile * small.chunk + small.tile + 6):
        check(small, n)
    for z in (0, 1, P - 1):
        check(small, small.tile * small.chunk + 1, z=z)
    lib = Shape()
    for n in boundary_sizes(lib.tile, lib.chunk, lib.e):
        check(lib, n)
    print("model_poly_scan: ok (tile %d, carry chunk %d)" % (lib.tile, lib.chunk))


if __name__ == "__main__":
    main()
