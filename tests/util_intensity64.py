"""Reference of the kernels in csrc/fsg_intensity.hip, of the GMM loop they share (csrc/fsg_common.h: fsg_randn4,
fsg_gmm_x4_loop) and of the GMM jobs of the one-launch sample head (csrc/fsg_deform.hip: sample_head_kernel, csrc/fsg_ride.h:
gmm_codes_job) for the tests (not a test module).

Plain numpy, one short function per operation; nothing here imports the product.  The only thing shared with another reference
is the integer Philox4x32-10 of oracle/fsg_keyed_draws.py, which tests/test_keyed_draws.py ties to the published Random123
known-answer vectors.

  normals64      the standard normals of stream (seed, stream_id) at arbitrary element indices, Box-Muller in float64
  gmm32          max(mu[l] + sigma[l] * z, 0) in the kernel's float32 operation order: BIT FOR BIT (the library is built without
                 FMA contraction, numpy's float32 arithmetic is IEEE)
  parts_label    the byte-wise sum of the per-meta-label volumes;  codes_label: the label of a code under a selection
  add_noise32    max(x + std * z, 0), float32, bit for bit
  gamma64        300 * (x / 300) ** g;  bias64: x * exp(trilinear(bias)) -- both through tests/util_warp64.epilogue64
  label_sums64   per-label count / sum / sum of squares in float64;  label_sums_bound: what label_stats_kernel may lose
  label_sums32   label_stats_kernel's own accumulation order restated in float32 (CPU tests of the bound)
  minmax_identities  the keys fsg_minmax_init writes
"""
import numpy as np

from oracle.fsg_keyed_draws import philox4x32_10
from tests.util_warp64 import epilogue64

F = np.float32
U32 = 2.0 ** -24       # unit roundoff of float32
NORMALS_ATOL = 4e-5    # tests/test_keyed_draws.py: the device's v_log / v_sqrt / v_sin / v_cos against numpy, |z| <= 5.77
BLOCK = 4096           # label_stats_kernel: voxels per workgroup (256 threads x 16 iterations)
TREE_LEVELS = 6        # the shuffle tree over 64 lanes
LDS_ADDS = 64          # 16 iterations x 4 waves: additions into one label's LDS cell per workgroup
KEY_POS_INF, KEY_NEG_INF = 0x7F800000, -2139095041  # fsg_f2key(+inf), fsg_f2key(-inf)
M32 = 0xFFFFFFFF


# ---- device normals (csrc/fsg_common.h: fsg_randn4, fsg_randn1) ------------------------------------------------------------
def philox_words(seed, stream_id, blocks, swap_counter=False):
    """The four words of the counter blocks `blocks` (uint64): counter = (block lo, block hi, stream lo, stream hi), key = (seed
    lo, seed hi).  swap_counter: the mutation of the CPU tests (stream and block words exchanged)."""
    b = np.asarray(blocks, dtype=np.uint64)
    seed, stream_id = int(seed), int(stream_id)
    c = [b & np.uint64(M32), b >> np.uint64(32), np.full(b.shape, stream_id & M32, np.uint64), np.full(b.shape, stream_id >> 32, np.uint64)]
    if swap_counter:
        c = [c[2], c[3], c[0], c[1]]
    return philox4x32_10(c[0], c[1], c[2], c[3], seed & M32, (seed >> 32) & M32)


def normals64(seed, stream_id, elements, lanes=(0, 1, 2, 3), swap_counter=False):
    """Element e is lane e & 3 of block e >> 2; a block is (r0 cos a0, r0 sin a0, r1 cos a1, r1 sin a1) with
    r = sqrt(-2 ln u), u = ((w >> 8) + 1) 2^-24 in (0, 1] from words x and z, a = 2 pi (w >> 8) 2^-24 from words y and w.
    float64 throughout.  lanes: the order of the four lanes (the CPU tests permute it as a mutation)."""
    e = np.asarray(elements, dtype=np.uint64)
    x, y, z, w = philox_words(seed, stream_id, e >> np.uint64(2), swap_counter)
    top = lambda v: (v >> np.uint64(8)).astype(np.float64)  # noqa: E731
    r0, r1 = np.sqrt(-2.0 * np.log((top(x) + 1.0) * U32)), np.sqrt(-2.0 * np.log((top(z) + 1.0) * U32))
    a0, a1 = 2.0 * np.pi * (top(y) * U32), 2.0 * np.pi * (top(w) * U32)
    four = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], -1)
    lane = np.asarray(lanes, dtype=np.int64)[(e & np.uint64(3)).astype(np.int64)]
    return np.take_along_axis(four, lane[..., None], -1)[..., 0]


def sample_indices(n, head=4096, tail=4101, strided=2 ** 16):
    """Every index of a small range; of a large one the first `head`, the last `tail` and `strided` at a stride."""
    if n <= head + tail + strided:
        return np.arange(n, dtype=np.int64)
    mid = head + (np.arange(strided, dtype=np.int64) * ((n - head - tail) // strided))
    return np.unique(np.concatenate([np.arange(head, dtype=np.int64), mid, np.arange(n - tail, n, dtype=np.int64)]))


# ---- K1: the GMM draw ----------------------------------------------------------------------------------------------------------
def _tables(mus, sigmas, ntab):
    mu, sg = np.zeros(256, F), np.zeros(256, F)
    mu[:ntab], sg[:ntab] = np.asarray(mus, F)[:ntab], np.asarray(sigmas, F)[:ntab]
    return mu, sg


def gmm32(labels, mus, sigmas, ntab, z, label_offset=0):
    """max(f32(mu[l] + f32(sigma[l] * z)), 0): two roundings.  l clamped to 0..255 in 64-bit arithmetic; the entries of the table
    from ntab on read as (0, 0), so the output there is 0 + 0 * z = +0 for every finite z.  A negative sum becomes +0; a -0 or NaN
    sum would stay (t < 0 is false), the tests produce neither.  label_offset: the mutation of the CPU tests."""
    l = np.clip(np.asarray(labels).astype(np.int64) + label_offset, 0, 255)
    mu, sg = _tables(mus, sigmas, ntab)
    z = np.asarray(z, dtype=F)
    p = sg[l] * z
    t = mu[l] + p
    assert p.dtype == F and t.dtype == F
    return np.where(t < 0, F(0), t).astype(F)


def parts_label(parts):
    """Byte-wise sum (mod 256) of the volumes that are given; None entries are absent."""
    out = None
    for p in parts:
        if p is not None:
            p = np.asarray(p, dtype=np.uint8)
            out = p.copy() if out is None else (out + p).astype(np.uint8)
    return out


def codes_label(codes, tuples, sel):
    """(row[sel0] + row[sel1] + row[sel2] + row[sel3]) & 255, row = tuples[code] (gmm_codes_job)."""
    t = np.asarray(tuples, dtype=np.int64)
    per_code = (t[:, sel[0]] + t[:, sel[1]] + t[:, sel[2]] + t[:, sel[3]]) & 255
    return per_code[np.asarray(codes, dtype=np.int64)].astype(np.uint8)


# ---- K5 / K8 stand-alone stages --------------------------------------------------------------------------------------------------
def add_noise32(x, std, z):
    """max(f32(x + f32(std * z)), 0), float32 (add_noise_kernel)."""
    x, z = np.asarray(x, dtype=F), np.asarray(z, dtype=F)
    t = x + F(std) * z
    assert t.dtype == F
    return np.where(t < 0, F(0), t).astype(F)


def gamma64(x, g):
    """300 * (x / 300) ** g in float64 on the float32 inputs (synthseg.py:274); NaN for x < 0 and a non-integer g."""
    return epilogue64(np.asarray(x, dtype=F), gamma=g)


def bias64(x, bias, tabs):
    """x * exp(bias interpolated x, then y, then z through the table entries), float64 (synthseg.py:178-182)."""
    return epilogue64(np.asarray(x, dtype=F), None, bias, tabs)


# ---- per-label statistics (label_stats_kernel) --------------------------------------------------------------------------------------
def label_sums64(labels, values, nlabels):
    """(count int64, sum, sum of squares) per label < nlabels; labels >= nlabels contribute nothing."""
    l = np.asarray(labels, dtype=np.int64).reshape(-1)
    v = np.asarray(values, dtype=F).astype(np.float64).reshape(-1)
    keep = l < nlabels
    cnt = np.bincount(l[keep], minlength=nlabels).astype(np.int64)
    return cnt, np.bincount(l[keep], weights=v[keep], minlength=nlabels), np.bincount(l[keep], weights=v[keep] ** 2, minlength=nlabels)


def label_sums_bound(labels, values, nlabels):
    """(bound of the sums, bound of the sums of squares), per label.

    From csrc/fsg_intensity.hip, label_stats_kernel: a workgroup handles 4096 consecutive voxels in 16 iterations of 256 threads.
    In an iteration, a wave peels the labels it sees one at a time.  For one label the 64 lanes hold v (or 0) and v * v (one
    rounding, float32) and add them up by `a += __shfl_xor(a, o)` for o = 32 .. 1: a balanced tree of depth 6, so every value
    passes through 6 rounded additions.  The leader then adds the wave's partial sum into the label's float32 LDS cell: at most
    16 iterations x 4 waves = 64 such additions per workgroup, in any order.  A value therefore passes through at most 6 + 64 = 70
    rounded additions (71 roundings for a square), each of a partial sum of magnitude <= the sum of |v| (of v^2) of that label in
    that workgroup:  70 u sum_block |v|  and  71 u sum_block v^2,  u = 2^-24.  Summed over the workgroups this is 70 u (71 u) of
    the label's sum of |v| (v^2) over the volume.  The LDS cell is then converted to double (exact) and added to the output by a
    double atomicAdd, one per workgroup and label: (workgroups) x 2^-53 of the same magnitude."""
    l = np.asarray(labels, dtype=np.int64).reshape(-1)
    v = np.abs(np.asarray(values, dtype=F).astype(np.float64).reshape(-1))
    keep = l < nlabels
    a1 = np.bincount(l[keep], weights=v[keep], minlength=nlabels)
    a2 = np.bincount(l[keep], weights=v[keep] ** 2, minlength=nlabels)
    nblk = (l.size + BLOCK - 1) // BLOCK
    return ((TREE_LEVELS + LDS_ADDS) * U32 + nblk * 2.0 ** -53) * a1, ((TREE_LEVELS + LDS_ADDS + 1) * U32 + nblk * 2.0 ** -53) * a2


def label_sums32(labels, values, nlabels, rs, drop_one_per_block=False):
    """label_stats_kernel's accumulation restated in float32: per workgroup, iteration and wave the tree over the 64 lanes
    (lane i + lane i ^ 32, then ^ 16, ... -- every lane ends with the same value, addition being commutative), then the wave
    partials of a label added sequentially into a float32 cell in an order shuffled by `rs` (the LDS atomics have no order),
    the cells added in float64.  drop_one_per_block: the deliberately wrong variant of the CPU tests (the largest |value| of
    every workgroup is left out)."""
    l = np.asarray(labels, dtype=np.int64).reshape(-1)
    v = np.asarray(values, dtype=F).reshape(-1)
    n = l.size
    s1, s2 = np.zeros(nlabels, np.float64), np.zeros(nlabels, np.float64)
    for b0 in range(0, n, BLOCK):
        lb, vb = l[b0:b0 + BLOCK], v[b0:b0 + BLOCK].copy()
        if drop_one_per_block:
            ok = np.flatnonzero(lb < nlabels)
            if ok.size:
                vb[ok[np.argmax(np.abs(vb[ok]))]] = 0
        pad = (-lb.size) % 64
        lw = np.concatenate([lb, np.full(pad, -1, np.int64)]).reshape(-1, 64)
        vw = np.concatenate([vb, np.zeros(pad, F)]).reshape(-1, 64)
        partial = {}
        for lrow, vrow in zip(lw, vw):
            for cur in np.unique(lrow[(lrow >= 0) & (lrow < nlabels)]):
                a = np.where(lrow == cur, vrow, F(0)).astype(F)
                q = np.where(lrow == cur, vrow * vrow, F(0)).astype(F)
                for o in (32, 16, 8, 4, 2, 1):
                    a, q = a[:o] + a[o:], q[:o] + q[o:]
                partial.setdefault(int(cur), []).append((a[0], q[0]))
        for cur, items in partial.items():
            ca, cq = F(0), F(0)
            for i in rs.permutation(len(items)):
                ca, cq = F(ca + items[i][0]), F(cq + items[i][1])
            s1[cur] += np.float64(ca)
            s2[cur] += np.float64(cq)
    return s1, s2


def minmax_identities(nmin, nmax):
    """What fsg_minmax_init (and the reset folded into fsg_gmm_sample_u8x4_mm) writes: nmin keys of +inf, then nmax of -inf."""
    return np.array([KEY_POS_INF] * nmin + [KEY_NEG_INF] * nmax, dtype=np.int32)


# ---- the inputs of the tests: the CPU tests of this reference and the GPU tests of the kernels draw them from here -------------------
RANDN_N = (1, 2, 3, 4, 5, 1023, 2 ** 23 + 5)  # the last: beyond 8192 workgroups x 256 lanes x 4, a second grid trip
RANDN_KEYS = ((0, 0), (1234, 7), (2 ** 63 + 5, 2 ** 40 + 3), (2 ** 64 - 1, 2 ** 64 - 1))  # (seed, stream_id)
I64_EDGES = (-1, -2 ** 40, 256, 2 ** 32 + 3, 2 ** 63 - 1)
STATS_N = (1, 63, 64, 65, 255, 256, 4095, 4096, 4097, 3 * 4096 + 1)
STATS_PATTERNS = ("one", "lanes64", "all256", "runs", "mixed")


def gmm_tables(ntab, seed=0):
    """(mus, sigmas): positive means (so that no sum is -0), entry 0 a plain 0 mean with a non-zero sigma."""
    rs = np.random.RandomState(1000 + ntab + seed)
    mus, sigmas = (rs.rand(ntab) * 225).astype(F), (5 + rs.rand(ntab) * 20).astype(F)
    mus[0] = 0
    return mus, sigmas


def gmm_labels(n, ntab, i64, seed=0):
    """Random labels 0..255 with the edges first (cycled when n is small): 0, ntab - 1, ntab, 255; int64 also I64_EDGES."""
    rs = np.random.RandomState(2000 + n % 1000 + ntab + seed)
    l = rs.randint(0, 256, n).astype(np.int64)
    edges = [0, ntab - 1, min(ntab, 255), 255] + (list(I64_EDGES) if i64 else [])
    k = min(n, len(edges))
    start = (n + ntab) % len(edges)  # a small n still meets every edge over the (n, ntab) grid
    l[:k] = [edges[(start + i) % len(edges)] for i in range(k)]
    if n > 2 * len(edges):
        l[-len(edges):] = edges     # and in the scalar tail
    return l if i64 else l.astype(np.uint8)


def gmm_noise(n, seed=0):
    """Injected normals: +0, -0, and values that drive mu + sigma z below 0."""
    rs = np.random.RandomState(3000 + n % 1000 + seed)
    z = (rs.randn(n) * 1.5).astype(F)
    for i, v in enumerate((0.0, -0.0, -60.0, 3.5, -1e-30)):
        if i < n:
            z[(i * 7 + n // 2) % n] = v
    return z


def split_parts(label, nparts, rs):
    """A uint8 label volume as `nparts` volumes with disjoint supports that add up to it."""
    label = np.asarray(label, dtype=np.uint8)
    owner = rs.randint(0, nparts, label.shape)
    return [np.where(owner == p, label, 0).astype(np.uint8) for p in range(nparts)]


def stats_inputs(n, pattern, nlabels, signed):
    """(labels uint8, values float32) of one label_stats_kernel case."""
    rs = np.random.RandomState(n % 1000 + 17 * STATS_PATTERNS.index(pattern) + nlabels + signed)
    e = np.arange(n)
    if pattern == "one":          # one label in every lane: one peel per wave
        l = np.full(n, min(7, nlabels - 1))
    elif pattern == "lanes64":    # 64 distinct labels in every wave: 64 peels
        l = e % 64
    elif pattern == "all256":
        l = e % 256
    elif pattern == "runs":       # piecewise constant, as a label map is
        l = np.repeat(rs.randint(0, min(nlabels + 6, 256), n), rs.randint(1, 300, n))[:n]
    else:                         # label 255 and labels >= nlabels in the same wave as valid ones
        l = np.array([0, 255, min(nlabels, 255), nlabels - 1, 254, 0, 1 % nlabels, 255])[e % 8]
    v = rs.rand(n) * 255
    if signed:
        v = v - 127.5
    return l.astype(np.uint8), v.astype(F)


def gamma_inputs(n):
    """[0, 255] with 0, two denormals, 1e-3, 300 and 255 in front (cycled with n so that n = 1 sees them too over the sizes)."""
    rs = np.random.RandomState(n % 1000)
    x = (rs.rand(n) * 255).astype(F)
    special = np.array([0.0, 1e-45, 1e-39, 1e-3, 300.0, 255.0], F)
    k = min(n, special.size)
    x[:k] = special[(n + np.arange(k)) % special.size]
    return x
