"""TEST INFRASTRUCTURE ONLY: the dropout masks of the HIP kernels, recomputed on the host.  numpy with uint64 arithmetic, no torch.

Every kernel that drops elements in training regenerates its mask in registers from philox4x32_10(counter, seed) of
csrc/common.h; nothing is stored.  This file restates that function and the two index rules the kernels' comments document, so
that a test can ask for the mask of a (seed, p, shape) without running any kernel.  The rules, with the lines they come from:

  philox4x32_10(ctr, seed)   csrc/common.h "Philox4x32-10 (Salmon et al.), counter = (ctr_lo, ctr_hi, 0, 0), key = seed": ten
                             rounds of (hi, lo) = 0xD2511F53 * c0, 0xCD9E8D57 * c2; c = (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0);
                             k0 += 0x9E3779B9, k1 += 0xBB67AE85 after every round.  Key words (seed_lo, seed_hi): the whole 64-bit
                             seed takes part.
  threshold(p)               csrc/common.h drop_threshold_host: "keep iff uniform(0,1) >= p  <=>  u32 >= p * 2^32".  p arrives as
                             the ABI's `float p_drop`, the product is taken in double and truncated, >= 2^32 - 1 caps at 0xFFFFFFFF.
  inv_keep(p)                every launcher: `1.0f / (1.0f - p)`, fp32 arithmetic on the fp32 p.
  keep32                     csrc/elementwise.hip keep4 ("Dropout masks are Philox4x32-10(seed, element index / 4)": call i4 gives
                             the words x, y, z, w to elements 4 i4 .. 4 i4 + 3, keep iff word >= thr); csrc/embed.hip keep_scale
                             ("one Philox call per 4 consecutive elements": call e >> 2, word e & 3); csrc/hie.hip keep4v ("the
                             draw of the flat element-wise kernels") and keep1 (call idx >> 2, word idx & 3).  The element index is
                             that of the LOGICAL contiguous tensor -- r * W + c for the 2-D kernels whatever the row strides,
                             (b * T + t) * H + h for vqf_dropout_bt whatever the layouts, the flat (N*L, E) / (N, T, L) index in
                             hie.hip.
  keep16                     csrc/fusion.hip keep_scale20: "elements e0 .. e0+19 are halfwords (e0 & 7) .. +19 of the 24-halfword
                             stream of calls e0/8, e0/8 + 1, e0/8 + 2", low half of a word first (`x & 0xFFFF` feeds sc[2k],
                             `x >> 16` sc[2k + 1]); keep iff halfword >= thr >> 16.  Flat: element e -> call e >> 3, halfword e & 7
                             of (x.lo, x.hi, y.lo, y.hi, z.lo, z.hi, w.lo, w.hi).  The element index is that of the (N*L, 5 O)
                             product of a QUESTION row (the grouped forms included: the image's P row is shared, the mask is not).

keep32 / keep16 take an element count or a shape and return a bool array of that shape: True = kept."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def _u64(x, n=None):
    a = np.asarray(x, dtype=np.uint64)
    return a if n is None else np.broadcast_to(a, (n,))


def philox4x32_10(ctr, seed, c2=0, c3=0):
    """ctr: an integer or an array of n 64-bit counters; seed: a 64-bit integer; c2, c3: the upper counter words (the library's are
    always 0; the published known-answer vectors use them) -> (n, 4) uint32, the words x, y, z, w of every call"""
    ctr = np.atleast_1d(np.asarray(ctr, dtype=np.uint64))
    n = ctr.shape[0]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    c0, c1 = ctr & MASK32, ctr >> S32
    c2, c3 = _u64(int(c2) & 0xFFFFFFFF, n), _u64(int(c3) & 0xFFFFFFFF, n)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                         # 32 x 32 -> 64: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> S32, p0 & MASK32, p1 >> S32, p1 & MASK32
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def threshold(p):
    """drop_threshold_host: floor(fp32(p) * 2^32) in double, capped at 0xFFFFFFFF"""
    t = float(np.float32(p)) * 4294967296.0
    return 0xFFFFFFFF if t >= 4294967295.0 else int(t)


def inv_keep(p):
    """the scale of a kept element: 1 / (1 - p) in fp32 arithmetic on the fp32 p -> np.float32"""
    p = np.float32(p)
    return np.float32(1.0) / (np.float32(1.0) - p)


def _count(n_or_shape):
    shape = (int(n_or_shape),) if np.isscalar(n_or_shape) else tuple(int(s) for s in n_or_shape)
    return shape, int(np.prod(shape, dtype=np.int64))


def words32(n, seed, first=0):
    """the 32-bit draws of elements first .. first + n - 1 (first % 4 == 0) -> (n,) uint32"""
    assert first % 4 == 0
    calls = np.arange(first // 4, first // 4 + (n + 3) // 4, dtype=np.uint64)
    return philox4x32_10(calls, seed).reshape(-1)[:n]


def words16(n, seed, first=0):
    """the 16-bit draws of elements first .. first + n - 1 (first % 8 == 0) -> (n,) uint32 holding 16-bit values"""
    assert first % 8 == 0
    calls = np.arange(first // 8, first // 8 + (n + 7) // 8, dtype=np.uint64)
    w = philox4x32_10(calls, seed)                        # (calls, 4)
    halves = np.stack([w & np.uint32(0xFFFF), w >> np.uint32(16)], axis=2)     # (calls, 4, 2): low half first
    return halves.reshape(-1)[:n]


def keep32(n_or_shape, seed, p, first=0):
    """the element-wise kernels' mask: element e keeps iff word e & 3 of call e >> 2 is >= threshold(p).  first: the flat index of
    the first element asked for (a multiple of 4): the tail of a long tensor without the head."""
    shape, n = _count(n_or_shape)
    return (words32(n, seed, first) >= np.uint32(threshold(p))).reshape(shape)


def keep16(n_or_shape, seed, p, first=0):
    """the fusion kernels' mask: element e keeps iff half-word e & 7 of call e >> 3 is >= threshold(p) >> 16"""
    shape, n = _count(n_or_shape)
    return (words16(n, seed, first) >= np.uint32(threshold(p) >> 16)).reshape(shape)
