"""Tensor-level wrappers over the C ABI (raw device pointers + current stream).

PyTorch is plumbing here: it owns device memory (caching allocator) and the
HIP stream; all arithmetic happens in libvqa_fusion.so.  There is no CPU
fallback -- a CPU tensor raises.
"""
import ctypes
import math
import torch

from . import lib as _l
from .grouping import SoftAnswers, check_soft_answers

GEMM_RELU = 1
GEMM_ACCUM = 2
POOL_K = 5


def _lib():
    return _l.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _l.VqfError("vqa fusion ops need GPU tensors (HIP extension is the only path; "
                              "no CPU fallback)")
        if t.dtype != torch.float32:
            raise _l.VqfError("fp32 tensor expected, got %s" % t.dtype)
        if not t.is_contiguous():
            raise _l.VqfError("contiguous tensor expected")


class _Workspace:
    """Grow-only scratch buffer per (device, stream): kernels on different streams may run
    concurrently (the image projection runs on a side stream), so they must not share slabs."""

    def __init__(self):
        self.bufs = {}

    def get(self, device, nbytes):
        nbytes = max(int(nbytes), 256)
        key = (device, torch.cuda.current_stream(device).cuda_stream)
        b = self.bufs.get(key)
        if b is None or b.numel() < nbytes:
            b = torch.empty(int(nbytes * 1.25) + 1024, dtype=torch.uint8, device=device)
            self.bufs[key] = b
        return b


_ws = _Workspace()
SPLITK_WS_BYTES = 192 << 20


def workspace(device, nbytes):
    return _ws.get(device, nbytes)


# ---------------------------------------------------------------------------
# library options (include/vqa_fusion.h VQF_OPT_*): process-wide launch policy, cached in the library
OPTIONS = {"gemm_f32_persist": 0, "gemm_bf16_persist": 1, "gemm_f32_loop": 2, "gemm_bf16_loop": 3, "gemm_f32_big": 4,
           "gemm_bf16_big": 5, "gemm_f32_wave": 6, "fuse_coal": 7, "fuse_ls": 8, "fuse_ls_bwd": 9, "gemm_cu_limit": 10,
           "gemm_f32_edge": 11, "gemm_f32_rounds": 12, "gemm_splitk_fused": 13, "gemm_f32_streamk": 14,
           "gemm_splitk_order": 15, "gemm_f32_sample": 16, "gemm_f32_n80": 17}


def set_option(name, value):
    """Set a library option (None / negative = the library's default); returns the value it replaced (-1 = default)."""
    prev = ctypes.c_int(0)
    _l.check(_lib().vqf_set_option(OPTIONS[name], -1 if value is None else int(value), ctypes.byref(prev)),
             "vqf_set_option(%s)" % name)
    return prev.value


def get_option(name):
    v = ctypes.c_int(0)
    _l.check(_lib().vqf_get_option(OPTIONS[name], ctypes.byref(v)), "vqf_get_option(%s)" % name)
    return v.value


STATS = {"gemm_f32_tile128": 0, "gemm_f32_big": 1, "gemm_f32_wave": 2, "gemm_bf16_tile128": 3, "gemm_bf16_big": 4,
         "gemm_f32_sample": 5, "gemm_f32_n80": 6}


def stat(name):
    """Launches routed to a GEMM kernel family since the library was loaded (include/vqa_fusion.h VQF_STAT_*)."""
    v = ctypes.c_longlong(0)
    _l.check(_lib().vqf_stat_get(STATS[name], ctypes.byref(v)), "vqf_stat_get(%s)" % name)
    return v.value


class options:
    """with ops.options(gemm_f32_persist=0): ...   sets the options for the block and restores what was there."""

    def __init__(self, **kw):
        self.kw, self.prev = kw, {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.prev[k] = set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            set_option(k, v)
        return False


def gemm(a, b, ta=False, tb=False, bias=None, relu=False, out=None, accumulate=False,
         M=None, N=None, K=None, splitk=True):
    """C[M,N] = Aop @ Bop^T (+bias) ; a/b are 2-D contiguous.

    ta=False: a is (M,K); ta=True: a is (K,M).   tb=False: b is (N,K); tb=True: b is (K,N).
    """
    _chk(bias)
    for t in (a, b, out):        # 2-D operands may be row-strided views (the ABI takes lda/ldb/ldc)
        if t is None:
            continue
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
            raise _l.VqfError("gemm: 2-D fp32 GPU tensors with contiguous rows expected")
    if M is None:
        M = a.shape[1] if ta else a.shape[0]
    if K is None:
        K = a.shape[0] if ta else a.shape[1]
        kb = b.shape[0] if tb else b.shape[1]
        if kb != K:
            raise _l.VqfError("gemm: inner dimensions differ (%d vs %d)" % (K, kb))
    if N is None:
        N = b.shape[1] if tb else b.shape[0]
    if out is None:
        if accumulate:
            raise _l.VqfError("gemm: accumulate needs out")
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    flags = (GEMM_RELU if relu else 0) | (GEMM_ACCUM if accumulate else 0)
    ws = None
    if splitk:
        ws = workspace(a.device, max(SPLITK_WS_BYTES, int(_lib().vqf_gemm_f32_ws_bytes(int(ta), int(tb), M, N, K))))
    rc = _lib().vqf_gemm_f32(int(ta), int(tb), M, N, K, _ptr(a), a.stride(0), _ptr(b), b.stride(0),
                             _ptr(out), out.stride(0), _ptr(bias), flags,
                             _ptr(ws), ws.numel() if ws is not None else 0, _stream())
    _l.check(rc, "vqf_gemm_f32")
    return out


def gemm_rows(a, b, L, tb=False, bias=None, relu=False, out=None):
    """C = a @ bop^T (+ bias) (relu) for a (NS*L, K) whose rows come in samples of L rows (the image regions of a sample): the
    per-sample-tile kernel (include/vqa_fusion.h vqf_gemm_f32_sample) where it takes the shape, vqf_gemm_f32 otherwise.
    b: (N, K), or (K, N) with tb; rows of a / b / out may be strided."""
    M, K = a.shape
    N = b.shape[1] if tb else b.shape[0]
    ok = (L > 0 and M % L == 0 and a.is_cuda and a.dtype == torch.float32 and b.dtype == torch.float32 and a.dim() == 2 and b.dim() == 2
          and a.stride(1) == 1 and b.stride(1) == 1 and (b.shape[0] if tb else b.shape[1]) == K
          and _lib().vqf_gemm_f32_sample_supported(M // L, L, N, K)
          and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0 and a.stride(0) % 4 == 0 and b.stride(0) % 4 == 0)
    if out is not None:
        ok = ok and out.dtype == torch.float32 and out.dim() == 2 and out.stride(1) == 1 and out.stride(0) % 2 == 0 and out.data_ptr() % 8 == 0
    if not ok:
        return gemm(a, b, tb=tb, bias=bias, relu=relu, out=out)
    _chk(bias)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    _l.check(_lib().vqf_gemm_f32_sample(int(bool(tb)), M // L, int(L), N, K, _ptr(a), a.stride(0), _ptr(b), b.stride(0), _ptr(out),
                                        out.stride(0), _ptr(bias), GEMM_RELU if relu else 0, _stream()), "vqf_gemm_f32_sample")
    return out


def gemm_rows_supported(NS, L, N, K):
    """whether gemm_rows runs (NS * L, K) x (N, K) products on the per-sample-tile kernel (include/vqa_fusion.h)"""
    return bool(_lib().vqf_gemm_f32_sample_supported(int(NS), int(L), int(N), int(K)))


def gemm_big_rows(ta, tb, M, N, K):
    """leading rows of an fp32 (ta, tb, M, N, K) product that run on the 256x256-tile kernel (M, 0, or the whole-rounds block of
    a mid-size shape: the other M - rows rows are a second launch): include/vqa_fusion.h vqf_gemm_f32_big_rows"""
    return int(_lib().vqf_gemm_f32_big_rows(int(bool(ta)), int(bool(tb)), int(M), int(N), int(K)))


def gemm_rowscale(a, b, rowscale, rows_per_scale, bias=None, relu=False):
    """C = relu?(rowscale[m // rows_per_scale] * (a @ b^T) + bias): a (M,K), b (N,K) fp32; the per-sample scale sits in the
    GEMM epilogue (the co-attention conv on the un-normalised fusion output)."""
    _chk(a, b, rowscale, bias)
    M, K = a.shape
    N = b.shape[0]
    if b.shape[1] != K or rowscale.numel() * rows_per_scale < M:
        raise _l.VqfError("gemm_rowscale: shape mismatch")
    out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    _l.check(_lib().vqf_gemm_f32_rowscale(0, 0, M, N, K, _ptr(a), a.stride(0), _ptr(b), b.stride(0), _ptr(out), N,
                                          _ptr(bias), GEMM_RELU if relu else 0, _ptr(rowscale), int(rows_per_scale),
                                          _stream()), "vqf_gemm_f32_rowscale")
    return out


def _chk_bf16(*ts):
    for t in ts:
        if not t.is_cuda or t.dtype != torch.bfloat16 or t.stride(-1) != 1:
            raise _l.VqfError("bf16 GPU tensor with contiguous rows expected")


K_PAD_ROWS = 32      # the large-tile bf16 GEMM takes K % 32 == 0: the row padding of a weight gradient's operands (regions_bf16)


def pad_rows(R, to=K_PAD_ROWS):
    return (R + to - 1) // to * to


def cast_bf16(x, pad_to=8, pad_rows_to=None):
    """fp32 (R,C) -> bf16 (R, C rounded up to a multiple of pad_to), zero-padded columns.
    pad_rows_to: the result has R rounded up to a multiple of it rows, rows R .. exact zeros (vqf_cast_f32_bf16_rows) -- an operand
    of a weight gradient whose K = R must be a multiple of 32; where R already is one this is the call without it."""
    _chk(x)
    R, C = x.shape
    Cp = (C + pad_to - 1) // pad_to * pad_to
    Rp = pad_rows(R, pad_rows_to) if pad_rows_to else R
    y = torch.empty((Rp, Cp), dtype=torch.bfloat16, device=x.device)
    if Rp != R:
        _l.check(_lib().vqf_cast_f32_bf16_rows(_ptr(x), R, C, x.stride(0), _ptr(y), Cp, Rp, _stream()), "vqf_cast_f32_bf16_rows")
        return y
    _l.check(_lib().vqf_cast_f32_bf16(_ptr(x), R, C, x.stride(0), _ptr(y), Cp, _stream()), "vqf_cast_f32_bf16")
    return y


GEMM_OUT_BF16 = 4


def gemm_bf16(a, b, ta=False, tb=False, bias=None, relu=False, M=None, N=None, K=None, out=None,
              accumulate=False, out_bf16=False):
    """C fp32 = Aop @ Bop^T with bf16 operands (row strides may exceed the logical widths).
    out_bf16: store C as bf16 (large-tile kernel only); returns None when that kernel does not apply."""
    _chk_bf16(a, b)
    _chk(bias)
    if out is not None:          # 2-D, rows may be strided (the ABI takes ldc)
        want = torch.bfloat16 if out_bf16 else torch.float32
        if not out.is_cuda or out.dtype != want or out.dim() != 2 or out.stride(1) != 1:
            raise _l.VqfError("gemm_bf16: out must be a 2-D %s GPU tensor with contiguous rows" % want)
    if M is None:
        M = a.shape[1] if ta else a.shape[0]
    if K is None:
        K = a.shape[0] if ta else a.shape[1]
    if N is None:
        N = b.shape[1] if tb else b.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=a.device)
    flags = (GEMM_RELU if relu else 0) | (GEMM_ACCUM if accumulate else 0) | (GEMM_OUT_BF16 if out_bf16 else 0)
    ws = workspace(a.device, max(SPLITK_WS_BYTES, int(_lib().vqf_gemm_bf16_ws_bytes(int(ta), int(tb), M, N, K))))
    rc = _lib().vqf_gemm_bf16(int(ta), int(tb), M, N, K, _ptr(a), a.stride(0), _ptr(b), b.stride(0),
                              _ptr(out), out.stride(0), _ptr(bias), flags, _ptr(ws), ws.numel(), _stream())
    if out_bf16 and rc == -3:          # VQF_E_UNSUPPORTED: shape outside the large-tile kernel -> caller uses fp32 output
        return None
    _l.check(rc, "vqf_gemm_bf16")
    return out


def gemm_bf16_rowscale(a, b, rowscale, rows_per_scale, bias=None, relu=False, K=None, M=None):
    """gemm_rowscale with bf16 operands: C fp32 = relu?(rowscale[m // rows_per_scale] * (a @ b^T) + bias), a (>=M, >=K), b (N, >=K)
    (M: the real rows of an a whose row count is padded, a weight gradient's K)"""
    _chk_bf16(a, b)
    _chk(rowscale, bias)
    N = b.shape[0]
    if M is None:
        M = a.shape[0]
    if K is None:
        K = a.shape[1]
    if b.shape[1] < K or a.shape[1] < K or a.shape[0] < M or M < 1 or rowscale.numel() * rows_per_scale < M:
        raise _l.VqfError("gemm_bf16_rowscale: shape mismatch")
    out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    _l.check(_lib().vqf_gemm_bf16_rowscale(0, 0, M, N, K, _ptr(a), a.stride(0), _ptr(b), b.stride(0), _ptr(out), N, _ptr(bias),
                                           GEMM_RELU if relu else 0, _ptr(rowscale), int(rows_per_scale), _stream()),
             "vqf_gemm_bf16_rowscale")
    return out


def _chk3(*ts):
    """3-D fp32 GPU operands of the batched GEMM: innermost dimension contiguous, row and batch strides free (column blocks
    of wider 2-D buffers viewed as (B, rows, cols))"""
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 3 or t.stride(2) != 1:
            raise _l.VqfError("bgemm: 3-D fp32 GPU tensors with a contiguous innermost dimension expected")


def bgemm(a, b, ta=False, tb=False, out=None, accumulate=False):
    """Batched: a (B,M,K)|(B,K,M), b (B,N,K)|(B,K,N) -> (B,M,N)."""
    _chk3(a, b, out)
    Bn = a.shape[0]
    M = a.shape[2] if ta else a.shape[1]
    K = a.shape[1] if ta else a.shape[2]
    N = b.shape[2] if tb else b.shape[1]
    kb = b.shape[1] if tb else b.shape[2]
    if kb != K or b.shape[0] != Bn:
        raise _l.VqfError("bgemm: shape mismatch")
    if out is None:
        out = torch.empty((Bn, M, N), dtype=torch.float32, device=a.device)
    rc = _lib().vqf_gemm_f32_batched(int(ta), int(tb), Bn, M, N, K, _ptr(a), a.stride(1), a.stride(0),
                                     _ptr(b), b.stride(1), b.stride(0), _ptr(out), out.stride(1),
                                     out.stride(0), GEMM_ACCUM if accumulate else 0, _stream())
    _l.check(rc, "vqf_gemm_f32_batched")
    return out


def colsum(x):
    _chk(x)
    M, N = x.shape
    out = torch.empty(N, dtype=torch.float32, device=x.device)
    need = _lib().vqf_colsum_ws_bytes(M, N)
    ws = workspace(x.device, need)
    _l.check(_lib().vqf_colsum_f32(_ptr(x), M, N, x.stride(0), _ptr(out), _ptr(ws), ws.numel(), _stream()),
             "vqf_colsum_f32")
    return out


def relu_bwd(dx, y, want_bias=True):
    _chk(dx, y)
    M, C = y.shape
    dpre = torch.empty_like(y)
    db = torch.empty(C, dtype=torch.float32, device=y.device) if want_bias else None
    ws = workspace(y.device, _lib().vqf_colsum_ws_bytes(M, C))
    _l.check(_lib().vqf_relu_bwd_f32(_ptr(dx), _ptr(y), M, C, _ptr(dpre), _ptr(db), _ptr(ws), ws.numel(),
                                     _stream()), "vqf_relu_bwd_f32")
    return dpre, db


def att_logits_fwd(hid, w2, b2):
    """logits (M,G) = hid (M,Hh) @ w2 (G,Hh)^T + b2; G in {1,2,3}."""
    _chk(hid, w2, b2)
    M, Hh = hid.shape
    G = w2.shape[0]
    out = torch.empty((M, G), dtype=torch.float32, device=hid.device)
    _l.check(_lib().vqf_att_logits_fwd(_ptr(hid), _ptr(w2), _ptr(b2), M, Hh, G, _ptr(out), _stream()),
             "vqf_att_logits_fwd")
    return out


def att_logits_fwd_lin(hid, w2, b2, b1):
    """-> (logits (M,G), lin (M,G)): lin = the part of the logit that is linear in the input of the ReLU layer in front
    (include/vqa_fusion.h vqf_att_logits_fwd_lin)."""
    _chk(hid, w2, b2, b1)
    M, Hh = hid.shape
    G = w2.shape[0]
    out = torch.empty((M, G), dtype=torch.float32, device=hid.device)
    lin = torch.empty((M, G), dtype=torch.float32, device=hid.device)
    _l.check(_lib().vqf_att_logits_fwd_lin(_ptr(hid), _ptr(w2), _ptr(b2), _ptr(b1), M, Hh, G, _ptr(out), _ptr(lin),
                                           _stream()), "vqf_att_logits_fwd_lin")
    return out, lin


def att_logits_bwd(dlogits, hid, w2, relu_mask=True, rowscale=None, rows_per_scale=1, out_bf16=False, pad_rows_to=None):
    """rowscale (per row group of rows_per_scale rows): the stored dhid_pre is scaled by it, the bias sums are not.
    out_bf16 (two glimpses, through the ReLU, Hh % 8 == 0): dhid_pre is stored as bf16 (the operand of the bf16 gradient GEMMs).
    pad_rows_to (out_bf16 only): dhid_pre has M rounded up to a multiple of it rows, exact zeros behind the M the kernel writes (the
    K padding of the layer's weight gradient on a region layout, as cast_bf16(pad_rows_to=))."""
    _chk(dlogits, hid, w2, rowscale)
    M, Hh = hid.shape
    G = w2.shape[0]
    dw2 = torch.empty((G, Hh), dtype=torch.float32, device=hid.device)
    db2 = torch.empty(G, dtype=torch.float32, device=hid.device)
    db1 = torch.empty(Hh, dtype=torch.float32, device=hid.device)
    ws = workspace(hid.device, _lib().vqf_att_logits_bwd_ws_bytes(M, Hh))
    if out_bf16:
        if not relu_mask or G != 2 or Hh % 8:
            raise _l.VqfError("att_logits_bwd: bf16 output needs the two-glimpse head through its ReLU and Hh % 8 == 0")
        dpre = torch.empty((pad_rows(M, pad_rows_to) if pad_rows_to else M, Hh), dtype=torch.bfloat16, device=hid.device)
        if dpre.shape[0] != M:
            dpre[M:].zero_()
        _l.check(_lib().vqf_att_logits_bwd_rowscale_obf16(_ptr(dlogits), _ptr(hid), _ptr(w2), _ptr(rowscale), int(rows_per_scale),
                                                          M, Hh, G, ctypes.c_void_p(dpre.data_ptr()), _ptr(dw2), _ptr(db2), _ptr(db1),
                                                          _ptr(ws), ws.numel(), _stream()), "vqf_att_logits_bwd_rowscale_obf16")
        return dpre, dw2, db2, db1
    dpre = torch.empty_like(hid)
    _l.check(_lib().vqf_att_logits_bwd_rowscale(_ptr(dlogits), _ptr(hid), _ptr(w2), _ptr(rowscale), int(rows_per_scale),
                                                M, Hh, G, int(bool(relu_mask)), _ptr(dpre), _ptr(dw2), _ptr(db2), _ptr(db1),
                                                _ptr(ws), ws.numel(), _stream()), "vqf_att_logits_bwd")
    return dpre, dw2, db2, db1


def _chk_lens(lens, N, what):
    """lens of the question-length forms (include/vqa_fusion.h *_len): None, or a contiguous (N,) int32 GPU tensor"""
    if lens is None:
        return
    if not lens.is_cuda or lens.dtype != torch.int32 or not lens.is_contiguous() or tuple(lens.shape) != (N,):
        raise _l.VqfError(what + ": lens must be a contiguous (N,) int32 GPU tensor")


def glimpse_pool_fwd(feat, logits, unit_softmax, pooled_out=None, lens=None):
    """feat (N,S,C) fp32 | bf16, logits (N*S,G) -> wts (N,G,S), pooled (N,G*C) (fp32; pooled_out: written there).
    lens (N) int32 (fp32 feat): the softmax runs over the first lens[n] positions, the weights beyond are exact zeros."""
    bf = feat.dtype == torch.bfloat16
    (_chk_bf16 if bf else _chk)(feat)
    if not feat.is_contiguous():
        raise _l.VqfError("contiguous feature tensor expected")
    _chk(logits)
    N, S, C = feat.shape
    G = logits.shape[1]
    wts = torch.empty((N, G, S), dtype=torch.float32, device=feat.device)
    if pooled_out is not None:
        _chk(pooled_out)
        if tuple(pooled_out.shape) != (N, G * C):
            raise _l.VqfError("glimpse_pool_fwd: pooled_out must be (N, G*C)")
        pooled = pooled_out
    else:
        pooled = torch.empty((N, G * C), dtype=torch.float32, device=feat.device)
    if lens is not None:
        if bf:
            raise _l.VqfError("glimpse_pool_fwd: lens with a bf16 feature tensor")
        _chk_lens(lens, N, "glimpse_pool_fwd")
        _l.check(_lib().vqf_glimpse_pool_fwd_len(_ptr(feat), _ptr(logits), _ptr(lens), N, S, C, G, int(bool(unit_softmax)),
                                                 _ptr(wts), _ptr(pooled), _stream()), "vqf_glimpse_pool_fwd_len")
        return wts, pooled
    fn = _lib().vqf_glimpse_pool_fwd_bf16 if bf else _lib().vqf_glimpse_pool_fwd
    _l.check(fn(_ptr(feat), _ptr(logits), N, S, C, G, int(bool(unit_softmax)), _ptr(wts), _ptr(pooled), _stream()),
             "vqf_glimpse_pool_fwd")
    return wts, pooled


def glimpse_pool_bwd(dpooled, feat, wts, unit_softmax, want_dfeat, dwts=None, lens=None):
    _chk(dpooled, wts, dwts)
    N, S, C = feat.shape
    G = wts.shape[1]
    dlogits = torch.empty((N * S, G), dtype=torch.float32, device=feat.device)
    if feat.dtype == torch.bfloat16:             # bf16 feature storage: the tensor is data
        _chk_bf16(feat)
        if want_dfeat or lens is not None:
            raise _l.VqfError("glimpse_pool_bwd: a bf16 feature tensor cannot receive a gradient or take lens")
        _l.check(_lib().vqf_glimpse_pool_bwd_bf16(_ptr(dpooled), _ptr(dwts), _ptr(feat), _ptr(wts), N, S, C, G,
                                                  int(bool(unit_softmax)), _ptr(dlogits), _stream()),
                 "vqf_glimpse_pool_bwd_bf16")
        return dlogits, None
    _chk(feat)
    dfeat = torch.empty_like(feat) if want_dfeat else None
    if lens is not None:                         # dlogits and dfeat of the positions >= lens[n] are exact zeros
        _chk_lens(lens, N, "glimpse_pool_bwd")
        _l.check(_lib().vqf_glimpse_pool_bwd_len(_ptr(dpooled), _ptr(dwts), _ptr(feat), _ptr(wts), _ptr(lens), N, S, C, G,
                                                 int(bool(unit_softmax)), _ptr(dlogits), _ptr(dfeat), _stream()),
                 "vqf_glimpse_pool_bwd_len")
        return dlogits, dfeat
    _l.check(_lib().vqf_glimpse_pool_bwd(_ptr(dpooled), _ptr(dwts), _ptr(feat), _ptr(wts), N, S, C, G,
                                         int(bool(unit_softmax)), _ptr(dlogits), _ptr(dfeat), _stream()),
             "vqf_glimpse_pool_bwd")
    return dlogits, dfeat


def dropout(x, keep=None, seed=0, p_drop=0.5, out=None):
    _chk(x, out)
    y = torch.empty_like(x) if out is None else out          # in place (out is x) allowed
    _l.check(_lib().vqf_dropout_f32(_ptr(x), _keep_ptr(keep), int(seed), float(p_drop), x.numel(), _ptr(y),
                                    _stream()), "vqf_dropout_f32")
    return y


def dropout_bt(x, out, keep=None, seed=0, p_drop=0.0, lens=None):
    """out[b,t,:] = x[b,t,:] * keep / (1 - p) for 3-D fp32 tensors of the same (B, T, H) shape with ANY strides on the first two
    axes (a transposed view in, a contiguous tensor out, or the other way round); the mask is indexed by (b, t, h).
    lens (B) int32: rows t >= lens[b] of out are zero."""
    for t_ in (x, out):
        if not t_.is_cuda or t_.dtype != torch.float32 or t_.dim() != 3 or t_.stride(2) != 1:
            raise _l.VqfError("dropout_bt: 3-D fp32 GPU tensors with a contiguous last axis expected")
    if x.shape != out.shape:
        raise _l.VqfError("dropout_bt: shapes differ")
    B, T, H = x.shape
    if lens is not None:
        _chk_lens(lens, B, "dropout_bt")
        _l.check(_lib().vqf_dropout_bt_len(_ptr(x), x.stride(0), x.stride(1), _keep_ptr(keep), int(seed), float(p_drop), _ptr(lens),
                                           B, T, H, _ptr(out), out.stride(0), out.stride(1), _stream()), "vqf_dropout_bt_len")
        return out
    _l.check(_lib().vqf_dropout_bt(_ptr(x), x.stride(0), x.stride(1), _keep_ptr(keep), int(seed), float(p_drop), B, T, H,
                                   _ptr(out), out.stride(0), out.stride(1), _stream()), "vqf_dropout_bt")
    return out


def tanh_dropout_fwd(a, b=None, keep=None, seed=0, p_drop=0.5, out=None):
    _chk(a, b, out)
    y = torch.empty_like(a) if out is None else out           # in place (out is a) allowed
    _l.check(_lib().vqf_tanh_dropout_fwd(_ptr(a), _ptr(b), _keep_ptr(keep), int(seed), float(p_drop),
                                         a.numel(), _ptr(y), _stream()), "vqf_tanh_dropout_fwd")
    return y


def tanh_dropout_bwd(dy, y, keep=None, seed=0, p_drop=0.5, out=None):
    _chk(dy, y, out)
    dx = torch.empty_like(y) if out is None else out          # in place (out is dy) allowed
    _l.check(_lib().vqf_tanh_dropout_bwd(_ptr(dy), _ptr(y), _keep_ptr(keep), int(seed), float(p_drop),
                                         y.numel(), _ptr(dx), _stream()), "vqf_tanh_dropout_bwd")
    return dx


def tanh_dropout_unpack_supported(U, R, L, E):
    return bool(_lib().vqf_tanh_dropout_unpack_supported(int(U), int(R), int(L), int(E)))


def _unpack_operands(name, roff, U, R, L, E):
    if not torch.is_tensor(roff) or not roff.is_cuda or roff.dtype != torch.int32 or not roff.is_contiguous() or \
            tuple(roff.shape) != (U + 1,):
        raise _l.VqfError("%s: roff must be a contiguous (U + 1,) = (%d,) int32 GPU tensor" % (name, U + 1))
    if not tanh_dropout_unpack_supported(U, R, L, E):
        raise _l.VqfError("%s: 1 <= U <= 65535 owners, 1 <= R < 2^29 rows, L <= 1024 and E %% 4 == 0, E <= 65536 are supported "
                          "(got U=%d, R=%d, L=%d, E=%d)" % (name, U, R, L, E))


def tanh_dropout_unpack_fwd(z, roff, U, L, keep=None, seed=0, p_drop=0.5):
    """z (R, E) packed rows, roff (U + 1) int32 -> y (U*L, E) padded: owner u's rows l < its count are dropout(tanh(z[start + l])),
    the others exact zeros (nothing read there).  Masks in the padded coordinates: keep (U*L, E), Philox index (u*L + l)*E + c."""
    _chk(z)
    if z.dim() != 2:
        raise _l.VqfError("tanh_dropout_unpack_fwd: z must be (R, E)")
    R, E = z.shape
    _unpack_operands("tanh_dropout_unpack_fwd", roff, U, R, L, E)
    if keep is not None and keep.numel() != U * L * E:
        raise _l.VqfError("tanh_dropout_unpack_fwd: keep must be (U*L, E) = (%d, %d)" % (U * L, E))
    y = torch.empty((U * L, E), dtype=torch.float32, device=z.device)
    _l.check(_lib().vqf_tanh_dropout_unpack_fwd(_ptr(z), _ptr(roff), _keep_ptr(keep), int(seed), float(p_drop), U, R, L, E, _ptr(y),
                                                _stream()), "vqf_tanh_dropout_unpack_fwd")
    return y


def tanh_dropout_pack_bwd(dy, y, roff, U, R, L, keep=None, seed=0, p_drop=0.5):
    """dy, y (U*L, E) padded, roff (U + 1) int32 -> dz (R, E) packed: the backward of tanh_dropout_unpack_fwd on the real rows; the
    padded rows of dy / y are not read."""
    _chk(dy, y)
    if y.dim() != 2 or y.shape[0] != U * L or dy.shape != y.shape:
        raise _l.VqfError("tanh_dropout_pack_bwd: dy and y must be (U*L, E)")
    E = y.shape[1]
    _unpack_operands("tanh_dropout_pack_bwd", roff, U, R, L, E)
    if keep is not None and keep.numel() != U * L * E:
        raise _l.VqfError("tanh_dropout_pack_bwd: keep must be (U*L, E) = (%d, %d)" % (U * L, E))
    dz = torch.empty((R, E), dtype=torch.float32, device=y.device)
    _l.check(_lib().vqf_tanh_dropout_pack_bwd(_ptr(dy), _ptr(y), _ptr(roff), _keep_ptr(keep), int(seed), float(p_drop), U, R, L, E,
                                              _ptr(dz), _stream()), "vqf_tanh_dropout_pack_bwd")
    return dz


def tanh_dropout_packed_fwd(z, roff, U, L, keep=None, seed=0, p_drop=0.5):
    """z (R, E) packed rows, roff (U + 1) int32 -> y (R, E) packed: row start + l is row u*L + l of tanh_dropout_unpack_fwd, bit
    for bit (masks in the padded coordinates: keep (U*L, E), Philox index (u*L + l)*E + c); no padded row exists."""
    _chk(z)
    if z.dim() != 2:
        raise _l.VqfError("tanh_dropout_packed_fwd: z must be (R, E)")
    R, E = z.shape
    _unpack_operands("tanh_dropout_packed_fwd", roff, U, R, L, E)
    if keep is not None and keep.numel() != U * L * E:
        raise _l.VqfError("tanh_dropout_packed_fwd: keep must be (U*L, E) = (%d, %d)" % (U * L, E))
    y = torch.empty((R, E), dtype=torch.float32, device=z.device)
    _l.check(_lib().vqf_tanh_dropout_packed_fwd(_ptr(z), _ptr(roff), _keep_ptr(keep), int(seed), float(p_drop), U, R, L, E, _ptr(y),
                                                _stream()), "vqf_tanh_dropout_packed_fwd")
    return y


def tanh_dropout_packed_bwd(dy, y, roff, U, L, keep=None, seed=0, p_drop=0.5):
    """dy, y (R, E) packed, roff (U + 1) int32 -> dz (R, E) packed: the backward of tanh_dropout_packed_fwd, the bits of
    tanh_dropout_pack_bwd on the padded operands."""
    _chk(dy, y)
    if y.dim() != 2 or dy.shape != y.shape:
        raise _l.VqfError("tanh_dropout_packed_bwd: dy and y must be (R, E)")
    R, E = y.shape
    _unpack_operands("tanh_dropout_packed_bwd", roff, U, R, L, E)
    if keep is not None and keep.numel() != U * L * E:
        raise _l.VqfError("tanh_dropout_packed_bwd: keep must be (U*L, E) = (%d, %d)" % (U * L, E))
    dz = torch.empty((R, E), dtype=torch.float32, device=y.device)
    _l.check(_lib().vqf_tanh_dropout_packed_bwd(_ptr(dy), _ptr(y), _ptr(roff), _keep_ptr(keep), int(seed), float(p_drop), U, R, L, E,
                                                _ptr(dz), _stream()), "vqf_tanh_dropout_packed_bwd")
    return dz


def tanh_bwd_rows_len(dy, y, lens, N, T, out=None):
    """dx = dy (1 - y^2) on the rows t < lens[n] of contiguous (N, T, L) tensors, zero on the others (in place allowed)"""
    _chk(dy, y, out)
    _chk_lens(lens, N, "tanh_bwd_rows_len")
    if y.numel() % (N * T) or dy.numel() != y.numel():
        raise _l.VqfError("tanh_bwd_rows_len: (N, T, L) tensors expected")
    dx = torch.empty_like(y) if out is None else out
    _l.check(_lib().vqf_tanh_bwd_rows_len(_ptr(dy), _ptr(y), _ptr(lens), int(N), int(T), y.numel() // (N * T), _ptr(dx), _stream()),
             "vqf_tanh_bwd_rows_len")
    return dx


def gate_tanh_sigmoid_fwd(a, b):
    """y = tanh(a) * sigmoid(b)   (modules.py:103-109)"""
    _chk(a, b)
    if a.shape != b.shape:
        raise _l.VqfError("gate_tanh_sigmoid: shapes differ")
    y = torch.empty_like(a)
    _l.check(_lib().vqf_gate_tanh_sigmoid_fwd(_ptr(a), _ptr(b), a.numel(), _ptr(y), _stream()), "vqf_gate_tanh_sigmoid_fwd")
    return y


def gate_tanh_sigmoid_bwd(dy, a, b):
    _chk(dy, a, b)
    da, db = torch.empty_like(a), torch.empty_like(b)
    _l.check(_lib().vqf_gate_tanh_sigmoid_bwd(_ptr(dy), _ptr(a), _ptr(b), a.numel(), _ptr(da), _ptr(db), _stream()),
             "vqf_gate_tanh_sigmoid_bwd")
    return da, db


def _chk2s(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
            raise _l.VqfError("2-D fp32 GPU tensor with contiguous rows expected")


def tanh_dropout_fwd2d(a, b=None, keep=None, seed=0, p_drop=0.5, out=None):
    """y = dropout(tanh(a + b)) over 2-D operands whose rows may be strided (column blocks of wider buffers); out may be b."""
    _chk2s(a, b, out)
    R, W = a.shape
    if out is None:
        out = torch.empty((R, W), dtype=torch.float32, device=a.device)
    _l.check(_lib().vqf_tanh_dropout_fwd2d(_ptr(a), a.stride(0), _ptr(b), b.stride(0) if b is not None else 0, _keep_ptr(keep),
                                           int(seed), float(p_drop), R, W, _ptr(out), out.stride(0), _stream()),
             "vqf_tanh_dropout_fwd2d")
    return out


def tanh_dropout_bwd2d(dy, y, keep=None, seed=0, p_drop=0.5, out=None):
    """dx = dy * keep / (1 - p) * (1 - tanh^2), 2-D operands with strided rows; out may be dy."""
    _chk2s(dy, y, out)
    R, W = y.shape
    if out is None:
        out = torch.empty((R, W), dtype=torch.float32, device=y.device)
    _l.check(_lib().vqf_tanh_dropout_bwd2d(_ptr(dy), dy.stride(0), _ptr(y), y.stride(0), _keep_ptr(keep), int(seed),
                                           float(p_drop), R, W, _ptr(out), out.stride(0), _stream()), "vqf_tanh_dropout_bwd2d")
    return out


def relu_bwd_rank1(dx, y, wts, dpooled, L, scale, want_bias=True, out=None):
    """dXpre = (dx + wts[m] * dpooled[m // L]) * (y > 0 ? scale : 0) (+ its column sums): include/vqa_fusion.h
    vqf_relu_bwd_rank1_f32.  out may be dx (in place)."""
    _chk(dx, y, wts, dpooled, out)
    M, C = y.shape
    dpre = torch.empty_like(y) if out is None else out
    db = torch.empty(C, dtype=torch.float32, device=y.device) if want_bias else None
    ws = workspace(y.device, _lib().vqf_colsum_ws_bytes(M, C))
    _l.check(_lib().vqf_relu_bwd_rank1_f32(_ptr(dx), _ptr(y), _ptr(wts), _ptr(dpooled), int(L), float(scale), M, C, _ptr(dpre),
                                           _ptr(db), _ptr(ws), ws.numel(), _stream()), "vqf_relu_bwd_rank1_f32")
    return dpre, db


def scale_by_device_scalar(x, s):
    """x (M,W) fp32 times the one-element GPU tensor s (a loss's incoming gradient), no host read: vqf_scale_rows with one scale
    for all rows"""
    _chk(x, s)
    if x.dim() != 2 or s.numel() != 1:
        raise _l.VqfError("scale_by_device_scalar: (M,W) tensor and a one-element scale expected")
    M, W = x.shape
    out = torch.empty_like(x)
    _l.check(_lib().vqf_scale_rows(_ptr(x), _ptr(s), M, M, W, _ptr(out), _stream()), "vqf_scale_rows")
    return out


def _ptr_array(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def multi_copy(pairs):
    """[(src, dst), ...] (<= 8 contiguous fp32 GPU tensors of equal size per pair): dst = src, ONE launch"""
    for a, b in pairs:
        _chk(a, b)
        if a.numel() != b.numel():
            raise _l.VqfError("multi_copy: sizes differ")
    n = (ctypes.c_longlong * len(pairs))(*[a.numel() for a, _ in pairs])
    _l.check(_lib().vqf_multi_copy_f32(_ptr_array([a for a, _ in pairs]), _ptr_array([b for _, b in pairs]), n, len(pairs),
                                       _stream()), "vqf_multi_copy_f32")


def multi_add(triples):
    """[(a, b, out), ...] (<= 4): out = a + b, ONE launch"""
    for a, b, o in triples:
        _chk(a, b, o)
        if not (a.numel() == b.numel() == o.numel()):
            raise _l.VqfError("multi_add: sizes differ")
    n = (ctypes.c_longlong * len(triples))(*[a.numel() for a, _, _ in triples])
    _l.check(_lib().vqf_multi_add_f32(_ptr_array([t[0] for t in triples]), _ptr_array([t[1] for t in triples]),
                                      _ptr_array([t[2] for t in triples]), n, len(triples), _stream()), "vqf_multi_add_f32")


# ---------------------------------------------------------------------------
# HieCoAtten's ladder as streaming passes (csrc/hie.hip; include/vqa_fusion.h vqf_hie_*)
def hie_stream_supported(N, L, E, T):
    return bool(_lib().vqf_hie_stream_supported(int(N), int(L), int(E), int(T)))


def hie_chunks(N, L):
    return int(_lib().vqf_hie_chunks(int(N), int(L)))


def _chk_ntl(u, N, T, L):
    _chk(u)
    if u.numel() != N * T * L:
        raise _l.VqfError("hie: the (N, T, L) coefficient tensor has the wrong size")


def _part_ld(part, E):
    """`part` of the streaming passes: (S, N*T, E) contiguous partial slabs, or -- one chunk per sample -- the 2-D destination
    of the final sums itself (rows may be strided) -> row pitch"""
    if part.dim() == 3:
        _chk(part)
        return E
    _chk2s(part)
    return part.stride(0)


def _part_add(part_add, S, what):
    """part_add of the region-count passes (one chunk per sample only): (N*T, E) rows the T-row sums are written on top of"""
    _chk2s(part_add)
    if part_add is not None and S != 1:
        raise _l.VqfError(what + ": part_add needs one chunk per sample")
    return _ptr(part_add), (part_add.stride(0) if part_add is not None else 0)


def hie_hv_fwd(a, C, V, drop, N, L, T, out, part, rlens=None, part_add=None):
    """out = dropout(tanh(a + C^T V)); part = the sums of C[t,l] a[l,:] over l: (S, N*T, E) per-chunk slabs, or (S == 1) the
    final (N*T, E) rows.  rlens (N) int32: the rows l >= rlens[n] of a and the columns of C there are not read, those rows of
    out are zero, part sums the real rows (every slab written); part_add (with rlens, S == 1): the sums land on top of it."""
    _chk2s(a, V, out)
    _chk_ntl(C, N, T, L)
    E = a.shape[1]
    keep, seed, p = drop
    if rlens is not None:
        _chk_lens(rlens, N, "hie_hv_fwd")
        pa, ldpa = _part_add(part_add, 1 if part.dim() == 2 else part.shape[0], "hie_hv_fwd")
        _l.check(_lib().vqf_hie_hv_fwd_regions(_ptr(a), a.stride(0), _ptr(C), _ptr(V), V.stride(0), _keep_ptr(keep), int(seed),
                                               float(p), _ptr(rlens), N, L, E, T, _ptr(out), out.stride(0), _ptr(part),
                                               _part_ld(part, E), pa, ldpa, _stream()), "vqf_hie_hv_fwd_regions")
        return out
    if part_add is not None:
        raise _l.VqfError("hie_hv_fwd: part_add comes with rlens")
    _l.check(_lib().vqf_hie_hv_fwd(_ptr(a), a.stride(0), _ptr(C), _ptr(V), V.stride(0), _keep_ptr(keep), int(seed), float(p),
                                   N, L, E, T, _ptr(out), out.stride(0), _ptr(part), _part_ld(part, E), _stream()), "vqf_hie_hv_fwd")
    return out


def hie_head_bwd(hv, dl, w, C, drop, N, L, T, out, part, wpart, part_add=None):
    """part_add (one chunk per sample only): the T-row sums are written on top of these (N*T, E) rows.
    wpart: (S*N, >= E + 4) partial rows, may be a column block of a wider buffer"""
    _chk2s(hv, out, part_add, wpart)
    _chk(dl, w)
    if wpart.shape[1] < hv.shape[1] + 4:
        raise _l.VqfError("hie_head_bwd: wpart rows hold E + 4 floats")
    _chk_ntl(C, N, T, L)
    E = hv.shape[1]
    keep, seed, p = drop
    _l.check(_lib().vqf_hie_head_bwd(_ptr(hv), hv.stride(0), _ptr(dl), _ptr(w), _ptr(C), _keep_ptr(keep), int(seed), float(p),
                                     N, L, E, T, _ptr(out), out.stride(0), _ptr(part), _part_ld(part, E), _ptr(part_add),
                                     part_add.stride(0) if part_add is not None else 0, _ptr(wpart), wpart.stride(0), _stream()),
             "vqf_hie_head_bwd")
    return out


def _colpart(colpart, N, L, E):
    """(S*N, E) column block the streaming pass writes one partial column-sum row per workgroup into -> (pointer, pitch)"""
    if colpart is None:
        return ctypes.c_void_p(0), 0
    _chk2s(colpart)
    if colpart.shape != (hie_chunks(N, L) * N, E):
        raise _l.VqfError("hie: colpart must be (chunks * N, E)")
    return _ptr(colpart), colpart.stride(0)


def hie_rank_add(a, U, V, N, L, T, out, colpart=None, rlens=None):
    """colpart: (S*N, E) rows (a column block of a wider buffer) receiving each workgroup's column sums of `out`.
    rlens (N) int32: rows l >= rlens[n] of a and columns of U there unread, those rows of out zero."""
    _chk2s(a, V, out)
    _chk_ntl(U, N, T, L)
    cp, ldcp = _colpart(colpart, N, L, a.shape[1])
    if rlens is not None:
        _chk_lens(rlens, N, "hie_rank_add")
        _l.check(_lib().vqf_hie_rank_add_regions(_ptr(a), a.stride(0), _ptr(U), _ptr(V), V.stride(0), _ptr(rlens), N, L, a.shape[1],
                                                 T, _ptr(out), out.stride(0), cp, ldcp, _stream()), "vqf_hie_rank_add_regions")
        return out
    _l.check(_lib().vqf_hie_rank_add(_ptr(a), a.stride(0), _ptr(U), _ptr(V), V.stride(0), N, L, a.shape[1], T, _ptr(out),
                                     out.stride(0), cp, ldcp, _stream()), "vqf_hie_rank_add")
    return out


def hie_rank_left(U, V, z, N, L, T, out, part, colpart=None, rlens=None, part_add=None):
    """out = U^T V; part = the sums of U[t,l] z[l,:] over l (as hie_hv_fwd's); rlens / part_add as in hie_hv_fwd (z for a)."""
    _chk2s(V, z, out)
    _chk_ntl(U, N, T, L)
    cp, ldcp = _colpart(colpart, N, L, z.shape[1])
    if rlens is not None:
        _chk_lens(rlens, N, "hie_rank_left")
        pa, ldpa = _part_add(part_add, 1 if part.dim() == 2 else part.shape[0], "hie_rank_left")
        _l.check(_lib().vqf_hie_rank_left_regions(_ptr(U), _ptr(V), V.stride(0), _ptr(z), z.stride(0), _ptr(rlens), N, L, z.shape[1],
                                                  T, _ptr(out), out.stride(0), _ptr(part), _part_ld(part, z.shape[1]), pa, ldpa,
                                                  cp, ldcp, _stream()), "vqf_hie_rank_left_regions")
        return out
    if part_add is not None:
        raise _l.VqfError("hie_rank_left: part_add comes with rlens")
    _l.check(_lib().vqf_hie_rank_left(_ptr(U), _ptr(V), V.stride(0), _ptr(z), z.stride(0), N, L, z.shape[1], T, _ptr(out),
                                      out.stride(0), _ptr(part), _part_ld(part, z.shape[1]), cp, ldcp, _stream()),
             "vqf_hie_rank_left")
    return out


def hie_affinity_supported(N, L, E, T, pairs=1):
    return bool(_lib().vqf_hie_affinity_supported(int(N), int(L), int(E), int(T), int(pairs)))


def _aff_operands(name, x1, y1, x2, y2, yprev, out, dims):
    """The operand checks of hie_affinity / hie_affinity_levels: x* 2-D with N*T rows, y* with N*L rows (rows may be strided);
    out (allocated here when None) and yprev contiguous with the elements of dims = (..., N, T, L).
    -> (out, row pitch of x2, row pitch of y2)"""
    _chk2s(x1, y1, x2, y2)
    N, T, L = dims[-3:]
    if x1.shape[0] != N * T or y1.shape[0] != N * L or (x2 is not None and (x2.shape[0] != N * T or y2.shape[0] != N * L)):
        raise _l.VqfError(name + ": operand shapes")
    if out is None:
        out = torch.empty(dims, dtype=torch.float32, device=x1.device)
    _chk(out, yprev)
    numel = math.prod(dims)
    if out.numel() != numel or (yprev is not None and yprev.numel() != numel):
        raise _l.VqfError(name + ": out / yprev must hold %s" % (dims,))
    return out, (x2.stride(0) if x2 is not None else 0), (y2.stride(0) if y2 is not None else 0)


def hie_affinity(x1, y1, N, L, T, x2=None, y2=None, epi=0, yprev=None, drop=(None, 0, 0.0), out=None, lens=None, rlens=None):
    """out (N, T, L) = epi(x1 y1^T [+ x2 y2^T]) per sample: x* rows n*T + t, y* rows n*L + l (2-D, rows may be strided).
    epi 0: the sums; 1: dropout(tanh(.)) with `drop` = (keep | None, seed, p); 2: the backward of epi 1 given its output yprev.
    lens (N) int32: rows t >= lens[n] of out are zero.  rlens (N) int32: columns l >= rlens[n] of out are zero, the y rows there
    (and yprev's columns) unread."""
    out, sx2, sy2 = _aff_operands("hie_affinity", x1, y1, x2, y2, yprev, out, (N, T, L))
    E = x1.shape[1]
    if y1.shape[1] != E or (x2 is not None and (x2.shape[1] != E or y2.shape[1] != E)):
        raise _l.VqfError("hie_affinity: operand shapes")
    keep, seed, p = drop
    if rlens is not None:
        _chk_lens(lens, N, "hie_affinity")
        _chk_lens(rlens, N, "hie_affinity")
        _l.check(_lib().vqf_hie_affinity_regions(_ptr(x1), x1.stride(0), _ptr(y1), y1.stride(0), _ptr(x2), sx2, _ptr(y2), sy2,
                                                 int(epi), _ptr(yprev), _keep_ptr(keep), int(seed), float(p), _ptr(lens), _ptr(rlens),
                                                 N, L, E, T, _ptr(out), _stream()), "vqf_hie_affinity_regions")
        return out
    if lens is not None:
        _chk_lens(lens, N, "hie_affinity")
        _l.check(_lib().vqf_hie_affinity_len(_ptr(x1), x1.stride(0), _ptr(y1), y1.stride(0), _ptr(x2), sx2, _ptr(y2), sy2, int(epi),
                                             _ptr(yprev), _keep_ptr(keep), int(seed), float(p), _ptr(lens), N, L, E, T, _ptr(out),
                                             _stream()), "vqf_hie_affinity_len")
        return out
    _l.check(_lib().vqf_hie_affinity(_ptr(x1), x1.stride(0), _ptr(y1), y1.stride(0), _ptr(x2), sx2, _ptr(y2), sy2, int(epi),
                                     _ptr(yprev), _keep_ptr(keep), int(seed), float(p), N, L, E, T, _ptr(out), _stream()),
             "vqf_hie_affinity")
    return out


def zero_cols_len(x, rlens, rows_per_sample, N, L):
    """x[r, l] = 0 for l >= rlens[(r // rows_per_sample) % N], in place: the padded columns of a contiguous (..., N, T, L) tensor
    (rows_per_sample = T): the ladder's C and dC on the batched-GEMM route"""
    _chk(x)
    _chk_lens(rlens, N, "zero_cols_len")
    if x.numel() % (rows_per_sample * N * L):
        raise _l.VqfError("zero_cols_len: a contiguous (G * N * rows_per_sample, L) tensor expected")
    _l.check(_lib().vqf_zero_cols_len(_ptr(x), _ptr(rlens), x.numel() // L, int(rows_per_sample), int(N), int(L), _stream()),
             "vqf_zero_cols_len")
    return x


def hie_slab_sum(part, out, add=None):
    """out[r,:] = (add[r,:] if add is given) + sum_s part[s, r, :]; part (S, R, W) contiguous, add / out 2-D, rows may be strided"""
    _chk(part)
    _chk2s(add, out)
    S, R, W = part.shape
    _l.check(_lib().vqf_hie_slab_sum(_ptr(part), S, R, W, _ptr(add), add.stride(0) if add is not None else 0, _ptr(out),
                                     out.stride(0), _stream()), "vqf_hie_slab_sum")
    return out


# ---------------------------------------------------------------------------
# the word / phrase / sentence ladder (csrc/hie_ladder.hip, the affinity in csrc/hie.hip; include/vqa_fusion.h vqf_phrase_ngram_*,
# vqf_hie_affinity_levels)
def phrase_ngram_supported(T, E):
    return bool(_lib().vqf_phrase_ngram_supported(int(T), int(E)))


def phrase_ngram_fwd(Z, bias, N, T, out=None, idx=None, lens=None):
    """Z (N*T, 6E) = Qw Wcat^T (rows may be strided), bias (3E) = [b1 | b2 | b3] -> (Qp (N*T, E), idx (N*T, E) uint8):
    Qp = tanh(max_k u_k), idx = the winning k - 1.  lens (N) int32: the windows stop at lens[n]; rows t >= lens[n]: Qp = 0, idx = 3"""
    _chk2s(Z, out)
    _chk(bias)
    E = Z.shape[1] // 6
    if Z.shape != (N * T, 6 * E) or bias.numel() != 3 * E:
        raise _l.VqfError("phrase_ngram_fwd: Z must be (N*T, 6E) and bias (3E)")
    if out is None:
        out = torch.empty((N * T, E), dtype=torch.float32, device=Z.device)
    if idx is None:
        idx = torch.empty((N * T, E), dtype=torch.uint8, device=Z.device)
    if lens is not None:
        _chk_lens(lens, N, "phrase_ngram_fwd")
        _l.check(_lib().vqf_phrase_ngram_fwd_len(_ptr(Z), Z.stride(0), _ptr(bias), _ptr(lens), int(N), int(T), int(E), _ptr(out),
                                                 out.stride(0), _ptr(idx), _stream()), "vqf_phrase_ngram_fwd_len")
        return out, idx
    _l.check(_lib().vqf_phrase_ngram_fwd(_ptr(Z), Z.stride(0), _ptr(bias), int(N), int(T), int(E), _ptr(out), out.stride(0),
                                         _ptr(idx), _stream()), "vqf_phrase_ngram_fwd")
    return out, idx


def phrase_ngram_bwd(dQp, Qp, idx, N, T, out=None, lens=None):
    """-> dZ (N*T, 6E): the gradient of Z gathered from du = dQp (1 - Qp^2) at the winning taps (lens: zero rows for t >= lens[n])"""
    _chk2s(dQp, Qp, out)
    E = Qp.shape[1]
    if not idx.is_cuda or idx.dtype != torch.uint8 or not idx.is_contiguous() or idx.shape != (N * T, E):
        raise _l.VqfError("phrase_ngram_bwd: idx must be a contiguous (N*T, E) uint8 GPU tensor")
    if out is None:
        out = torch.empty((N * T, 6 * E), dtype=torch.float32, device=Qp.device)
    if lens is not None:
        _chk_lens(lens, N, "phrase_ngram_bwd")
        _l.check(_lib().vqf_phrase_ngram_bwd_len(_ptr(dQp), dQp.stride(0), _ptr(Qp), Qp.stride(0), _ptr(idx), _ptr(lens), int(N), int(T),
                                                 int(E), _ptr(out), out.stride(0), _stream()), "vqf_phrase_ngram_bwd_len")
        return out
    _l.check(_lib().vqf_phrase_ngram_bwd(_ptr(dQp), dQp.stride(0), _ptr(Qp), Qp.stride(0), _ptr(idx), int(N), int(T), int(E),
                                         _ptr(out), out.stride(0), _stream()), "vqf_phrase_ngram_bwd")
    return out


def hie_affinity_levels_supported(N, L, E, T, G, pairs=1):
    return bool(_lib().vqf_hie_affinity_levels_supported(int(N), int(L), int(E), int(T), int(G), int(pairs)))


def hie_affinity_levels(x1, lvx1, y1, lvy1, G, N, L, T, E, x2=None, lvx2=0, y2=None, lvy2=0, epi=0, yprev=None, out=None,
                        lens=None, rlens=None):
    """out (G, N, T, L): level g = epi(X1_g Y1_g^T [+ X2_g Y2_g^T]) per sample, X_g = the E columns of x at offset g * lvx (rows
    n*T + t), Y_g those of y at g * lvy (rows n*L + l; lvy = 0: one y shared by the levels).  2-D operands, rows may be strided.
    epi 0: the sums; 1: tanh; 2: sums * (1 - yprev^2).  lens (N) int32: rows t >= lens[n] of every level are zero; rlens (N)
    int32: columns l >= rlens[n] of every level are zero, the y rows there unread."""
    out, sx2, sy2 = _aff_operands("hie_affinity_levels", x1, y1, x2, y2, yprev, out, (G, N, T, L))
    if rlens is not None:
        _chk_lens(lens, N, "hie_affinity_levels")
        _chk_lens(rlens, N, "hie_affinity_levels")
        _l.check(_lib().vqf_hie_affinity_levels_regions(_ptr(x1), x1.stride(0), int(lvx1), _ptr(y1), y1.stride(0), int(lvy1),
                                                        _ptr(x2), sx2, int(lvx2), _ptr(y2), sy2, int(lvy2), int(G), int(epi),
                                                        _ptr(yprev), _ptr(lens), _ptr(rlens), int(N), int(L), int(E), int(T),
                                                        _ptr(out), _stream()), "vqf_hie_affinity_levels_regions")
        return out
    if lens is not None:
        _chk_lens(lens, N, "hie_affinity_levels")
        _l.check(_lib().vqf_hie_affinity_levels_len(_ptr(x1), x1.stride(0), int(lvx1), _ptr(y1), y1.stride(0), int(lvy1),
                                                    _ptr(x2), sx2, int(lvx2), _ptr(y2), sy2, int(lvy2), int(G), int(epi), _ptr(yprev),
                                                    _ptr(lens), int(N), int(L), int(E), int(T), _ptr(out), _stream()),
                 "vqf_hie_affinity_levels_len")
        return out
    _l.check(_lib().vqf_hie_affinity_levels(_ptr(x1), x1.stride(0), int(lvx1), _ptr(y1), y1.stride(0), int(lvy1),
                                            _ptr(x2), sx2, int(lvx2), _ptr(y2), sy2, int(lvy2), int(G), int(epi), _ptr(yprev),
                                            int(N), int(L), int(E), int(T), _ptr(out), _stream()), "vqf_hie_affinity_levels")
    return out


# the guided attention logits of the ladder's alternating co-attention (csrc/hie_ladder_alt.hip; include/vqa_fusion.h
# vqf_guided_logits_*)
def guided_logits_supported(N, S, E, G):
    return bool(_lib().vqf_guided_logits_supported(int(N), int(S), int(E), int(G)))


def _guided_operands(name, xh, gp, w, N, S):
    _chk2s(xh)
    _chk(gp, w)
    G, E = w.shape
    if xh.shape[0] != N * S or xh.shape[1] != G * E or (gp is not None and tuple(gp.shape) != (N, G * E)):
        raise _l.VqfError(name + ": xh must be (N*S, G*E), gp (N, G*E) or None, w (G, E)")
    if not guided_logits_supported(N, S, E, G):
        raise _l.VqfError(name + ": E %% 32 == 0, E <= 1024, 1 <= S <= 1024, G in {1, 2, 3} and N <= 65535 are supported "
                          "(got N=%d, S=%d, E=%d, G=%d)" % (N, S, E, G))
    return G, E


def guided_logits_fwd(xh, gp, w, N, S):
    """xh (N*S, G*E) (rows may be strided: a column block of a wider buffer), gp (N, G*E) or None, w (G, E) ->
    logits (N*S, G) = sum_e w[g, e] tanh(xh[r, g*E + e] + gp[r // S, g*E + e]); the hidden activation is not stored."""
    G, E = _guided_operands("guided_logits_fwd", xh, gp, w, N, S)
    out = torch.empty((N * S, G), dtype=torch.float32, device=xh.device)
    _l.check(_lib().vqf_guided_logits_fwd(_ptr(xh), xh.stride(0), _ptr(gp), _ptr(w), int(N), int(S), E, G, _ptr(out), _stream()),
             "vqf_guided_logits_fwd")
    return out


def guided_logits_bwd(dlogits, xh, gp, w, N, S, out=None):
    """-> (dxh (N*S, G*E) (out: written there, rows may be strided), dgp (N, G*E) = the per-sample row sums of dxh (also when
    gp is None: its column sum is the bias gradient of the layer that made xh), dw (G, E)); fixed summation order."""
    G, E = _guided_operands("guided_logits_bwd", xh, gp, w, N, S)
    _chk(dlogits)
    _chk2s(out)
    if tuple(dlogits.shape) != (N * S, G) or (out is not None and tuple(out.shape) != (N * S, G * E)):
        raise _l.VqfError("guided_logits_bwd: dlogits must be (N*S, G) and out (N*S, G*E)")
    if out is None:
        out = torch.empty((N * S, G * E), dtype=torch.float32, device=xh.device)
    dgp = torch.empty((N, G * E), dtype=torch.float32, device=xh.device)
    dw = torch.empty((G, E), dtype=torch.float32, device=xh.device)
    ws = workspace(xh.device, _lib().vqf_guided_logits_bwd_ws_bytes(int(N), int(S), E, G))
    _l.check(_lib().vqf_guided_logits_bwd(_ptr(dlogits), _ptr(xh), xh.stride(0), _ptr(gp), _ptr(w), int(N), int(S), E, G, _ptr(out),
                                          out.stride(0), _ptr(dgp), _ptr(dw), _ptr(ws), ws.numel(), _stream()),
             "vqf_guided_logits_bwd")
    return out, dgp, dw


# the grouped forms: N questions over U shared images (include/vqa_fusion.h "The grouped forms"; host/grouping.py::_group_index
# makes idx / order / grp_off).  The kernels clamp what the index arrays hold; only their type, shape and device are checked here.
def _chk_group(name, N, U, idx=None, order=None, grp_off=None):
    for t, shape, what in ((idx, (N,), "idx"), (order, (N,), "order"), (grp_off, (U + 1,), "grp_off")):
        if t is None:
            continue
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or tuple(t.shape) != shape:
            raise _l.VqfError("%s: %s must be a contiguous %s int32 GPU tensor" % (name, what, shape))


def guided_logits_grouped_supported(N, U, S, E, G):
    return bool(_lib().vqf_guided_logits_grouped_supported(int(N), int(U), int(S), int(E), int(G)))


def _guided_grouped_operands(name, xh, gp, w, N, U, S):
    _chk2s(xh)
    _chk(gp, w)
    G, E = w.shape
    if gp is None or xh.shape[0] != U * S or xh.shape[1] != G * E or tuple(gp.shape) != (N, G * E):
        raise _l.VqfError(name + ": xh must be (U*S, G*E), gp (N, G*E), w (G, E)")
    if not guided_logits_grouped_supported(N, U, S, E, G):
        raise _l.VqfError(name + ": E %% 32 == 0, E <= 1024, 1 <= S <= 1024, G in {1, 2, 3}, N <= 65535 and U <= 65535 are "
                          "supported (got N=%d, U=%d, S=%d, E=%d, G=%d)" % (N, U, S, E, G))
    return G, E


def guided_logits_fwd_grouped(xh, gp, w, idx, N, U, S):
    """xh (U*S, G*E) (rows may be strided), gp (N, G*E), w (G, E), idx (N) int32 -> logits (N*S, G): question n reads the xh
    rows of image idx[n] (clamped to [0, U - 1] in the kernel) and its own guidance row."""
    G, E = _guided_grouped_operands("guided_logits_fwd_grouped", xh, gp, w, N, U, S)
    _chk_group("guided_logits_fwd_grouped", N, U, idx=idx)
    out = torch.empty((N * S, G), dtype=torch.float32, device=xh.device)
    _l.check(_lib().vqf_guided_logits_fwd_grouped(_ptr(xh), xh.stride(0), _ptr(gp), _ptr(w), _ptr(idx), int(N), int(U), int(S), E, G,
                                                  _ptr(out), _stream()), "vqf_guided_logits_fwd_grouped")
    return out


def guided_logits_bwd_grouped(dlogits, xh, gp, w, order, grp_off, N, U, S, out=None):
    """-> (dxh (U*S, G*E) = the sum over each image's questions (out: written there, rows may be strided; an image without a
    question gets zero rows), dgp (N, G*E), dw (G, E)); the questions of a group are added in `order`: fixed summation order."""
    G, E = _guided_grouped_operands("guided_logits_bwd_grouped", xh, gp, w, N, U, S)
    _chk_group("guided_logits_bwd_grouped", N, U, order=order, grp_off=grp_off)
    _chk(dlogits)
    _chk2s(out)
    if tuple(dlogits.shape) != (N * S, G) or (out is not None and tuple(out.shape) != (U * S, G * E)):
        raise _l.VqfError("guided_logits_bwd_grouped: dlogits must be (N*S, G) and out (U*S, G*E)")
    if out is None:
        out = torch.empty((U * S, G * E), dtype=torch.float32, device=xh.device)
    dgp = torch.empty((N, G * E), dtype=torch.float32, device=xh.device)
    dw = torch.empty((G, E), dtype=torch.float32, device=xh.device)
    ws = workspace(xh.device, _lib().vqf_guided_logits_bwd_grouped_ws_bytes(int(N), int(U), int(S), E, G))
    _l.check(_lib().vqf_guided_logits_bwd_grouped(_ptr(dlogits), _ptr(xh), xh.stride(0), _ptr(gp), _ptr(w), _ptr(order), _ptr(grp_off),
                                                  int(N), int(U), int(S), E, G, _ptr(out), out.stride(0), _ptr(dgp), _ptr(dw),
                                                  _ptr(ws), ws.numel(), _stream()), "vqf_guided_logits_bwd_grouped")
    return out, dgp, dw


def glimpse_pool_grouped_supported(N, U, S, C, G):
    return bool(_lib().vqf_glimpse_pool_grouped_supported(int(N), int(U), int(S), int(C), int(G)))


def _pool_grouped_dims(name, feat, G, N):
    _chk(feat)
    U, S, C = feat.shape
    if not glimpse_pool_grouped_supported(N, U, S, C, G):
        raise _l.VqfError(name + ": N <= 65535, U <= 65535, S <= 1024, C %% 4 == 0 and G in {1, 2, 3} are supported "
                          "(got N=%d, U=%d, S=%d, C=%d, G=%d)" % (N, U, S, C, G))
    return U, S, C


def glimpse_pool_fwd_grouped(feat, logits, idx, lens=None):
    """feat (U, S, C), logits (N*S, G), idx (N) int32 -> wts (N, G, S), pooled (N, G*C): question n pools the rows of image idx[n].
    lens (N) int32 per QUESTION: the softmax runs over the first lens[n] rows, the weights beyond are exact zeros."""
    _chk(logits)
    N, G = idx.shape[0], logits.shape[1]
    U, S, C = _pool_grouped_dims("glimpse_pool_fwd_grouped", feat, G, N)
    _chk_group("glimpse_pool_fwd_grouped", N, U, idx=idx)
    if logits.shape[0] != N * S:
        raise _l.VqfError("glimpse_pool_fwd_grouped: logits must be (N*S, G)")
    wts = torch.empty((N, G, S), dtype=torch.float32, device=feat.device)
    pooled = torch.empty((N, G * C), dtype=torch.float32, device=feat.device)
    if lens is not None:
        _chk_lens(lens, N, "glimpse_pool_fwd_grouped")
        _l.check(_lib().vqf_glimpse_pool_fwd_grouped_len(_ptr(feat), _ptr(logits), _ptr(idx), _ptr(lens), N, U, S, C, G, _ptr(wts),
                                                         _ptr(pooled), _stream()), "vqf_glimpse_pool_fwd_grouped_len")
        return wts, pooled
    _l.check(_lib().vqf_glimpse_pool_fwd_grouped(_ptr(feat), _ptr(logits), _ptr(idx), N, U, S, C, G, _ptr(wts), _ptr(pooled),
                                                 _stream()), "vqf_glimpse_pool_fwd_grouped")
    return wts, pooled


def glimpse_pool_bwd_grouped(dpooled, feat, wts, idx, order, grp_off, want_dfeat, dwts=None, lens=None):
    """dpooled (N, G*C), feat (U, S, C), wts (N, G, S) -> (dlogits (N*S, G), dfeat (U, S, C) or None): dfeat[u] sums the questions
    of image u in `order` (fixed summation order; zero rows for an image without a question)."""
    _chk(dpooled, wts, dwts)
    N, G, S_ = wts.shape
    U, S, C = _pool_grouped_dims("glimpse_pool_bwd_grouped", feat, G, N)
    _chk_group("glimpse_pool_bwd_grouped", N, U, idx=idx, order=order, grp_off=grp_off)
    if S_ != S or tuple(dpooled.shape) != (N, G * C) or (dwts is not None and tuple(dwts.shape) != (N, G, S)):
        raise _l.VqfError("glimpse_pool_bwd_grouped: dpooled must be (N, G*C), wts and dwts (N, G, S)")
    dlogits = torch.empty((N * S, G), dtype=torch.float32, device=feat.device)
    dfeat = torch.empty_like(feat) if want_dfeat else None
    if lens is not None:                         # (N) per question: dlogits of the positions >= lens[n] are exact zeros
        _chk_lens(lens, N, "glimpse_pool_bwd_grouped")
        _l.check(_lib().vqf_glimpse_pool_bwd_grouped_len(_ptr(dpooled), _ptr(dwts), _ptr(feat), _ptr(wts), _ptr(idx), _ptr(order),
                                                         _ptr(grp_off), _ptr(lens), N, U, S, C, G, _ptr(dlogits), _ptr(dfeat),
                                                         _stream()), "vqf_glimpse_pool_bwd_grouped_len")
        return dlogits, dfeat
    _l.check(_lib().vqf_glimpse_pool_bwd_grouped(_ptr(dpooled), _ptr(dwts), _ptr(feat), _ptr(wts), _ptr(idx), _ptr(order),
                                                 _ptr(grp_off), N, U, S, C, G, _ptr(dlogits), _ptr(dfeat), _stream()),
             "vqf_glimpse_pool_bwd_grouped")
    return dlogits, dfeat


def row_block_supported(N, U, blk):
    return bool(_lib().vqf_row_block_supported(int(N), int(U), int(blk)))


def row_block_gather(src, idx):
    """src (U, ...) contiguous, idx (N) int32 -> (N, ...) = src[idx] (idx clamped to [0, U - 1] in the kernel)."""
    _chk(src)
    if not torch.is_tensor(idx) or idx.dim() != 1:
        raise _l.VqfError("row_block_gather: idx must be a contiguous (N,) int32 GPU tensor")
    U, N = src.shape[0], idx.shape[0]
    blk = src[0].numel()
    _chk_group("row_block_gather", N, U, idx=idx)
    if not row_block_supported(N, U, blk):
        raise _l.VqfError("row_block_gather: N <= 65535, U <= 65535 and a block of a multiple of 4 floats are supported "
                          "(got N=%d, U=%d, block=%d)" % (N, U, blk))
    out = torch.empty((N,) + tuple(src.shape[1:]), dtype=torch.float32, device=src.device)
    _l.check(_lib().vqf_row_block_gather(_ptr(src), _ptr(idx), N, U, blk, _ptr(out), _stream()), "vqf_row_block_gather")
    return out


def row_block_group_sum(src, order, grp_off):
    """src (N, ...) contiguous -> (U, ...): out[u] = the sum of the blocks order[grp_off[u]] .. order[grp_off[u + 1] - 1], added in
    that order (the backward of row_block_gather; an empty group gives zeros)."""
    _chk(src)
    N, U = src.shape[0], grp_off.shape[0] - 1
    blk = src[0].numel()
    _chk_group("row_block_group_sum", N, U, order=order, grp_off=grp_off)
    if not row_block_supported(N, U, blk):
        raise _l.VqfError("row_block_group_sum: N <= 65535, U <= 65535 and a block of a multiple of 4 floats are supported "
                          "(got N=%d, U=%d, block=%d)" % (N, U, blk))
    out = torch.empty((U,) + tuple(src.shape[1:]), dtype=torch.float32, device=src.device)
    _l.check(_lib().vqf_row_block_group_sum(_ptr(src), _ptr(order), _ptr(grp_off), N, U, blk, _ptr(out), _stream()),
             "vqf_row_block_group_sum")
    return out


def softmax_rows_fwd(x):
    _chk(x)
    R, W = x.shape
    y = torch.empty_like(x)
    _l.check(_lib().vqf_softmax_rows_fwd(_ptr(x), R, W, _ptr(y), _stream()), "vqf_softmax_rows_fwd")
    return y


def softmax_rows_bwd(dy, y):
    _chk(dy, y)
    R, W = y.shape
    dx = torch.empty_like(y)
    _l.check(_lib().vqf_softmax_rows_bwd(_ptr(dy), _ptr(y), R, W, _ptr(dx), _stream()), "vqf_softmax_rows_bwd")
    return dx


def log_softmax_rows_fwd(x):
    _chk(x)
    R, W = x.shape
    y = torch.empty_like(x)
    _l.check(_lib().vqf_log_softmax_rows_fwd(_ptr(x), R, W, _ptr(y), _stream()), "vqf_log_softmax_rows_fwd")
    return y


def log_softmax_rows_bwd(dy, y):
    _chk(dy, y)
    R, W = y.shape
    dx = torch.empty_like(y)
    _l.check(_lib().vqf_log_softmax_rows_bwd(_ptr(dy), _ptr(y), R, W, _ptr(dx), _stream()), "vqf_log_softmax_rows_bwd")
    return dx


def _keep_ptr(keep):
    if keep is None:
        return ctypes.c_void_p(0)
    if not keep.is_cuda or keep.dtype != torch.uint8 or not keep.is_contiguous():
        raise _l.VqfError("keep mask must be a contiguous uint8 GPU tensor")
    return ctypes.c_void_p(keep.data_ptr())


def _l2_norm_tail(R, rowssq, N, L, O, normalise):
    """The tail of every mfb_fuse_fwd*: norm / inv of each sample from the rows' partial sums of squares (four per row) and, with
    normalise, R scaled by inv in place -> (norm (N), inv (N))."""
    norm = torch.empty(N, dtype=torch.float32, device=R.device)
    inv = torch.empty(N, dtype=torch.float32, device=R.device)
    _l.check(_lib().vqf_l2_group_norm(_ptr(rowssq), N, 4 * L, _ptr(norm), _ptr(inv), _stream()), "vqf_l2_group_norm")
    if normalise:
        _l.check(_lib().vqf_scale_rows(_ptr(R), _ptr(inv), N * L, L, O, _ptr(R), _stream()), "vqf_scale_rows")
    return norm, inv


def _l2_norm_bwd_coefs(dY, Y, norm, inv, N, L, O, lin):
    """The head of every mfb_fuse_bwd*: the two per-sample coefficients of the L2 norm's backward -> (cA (N), cB (N), the inv the
    fusion backward takes).  lin = (dlogits, lin) of the consumer's attention head (mfb_fuse_bwd): sum(R * dYs) from its (N*L, G)
    tensors and inv = 1; otherwise a rowdot pass over the (N*L, O) ones."""
    dev = Y.device
    cA = torch.empty(N, dtype=torch.float32, device=dev)
    cB = torch.empty(N, dtype=torch.float32, device=dev)
    if lin is not None:
        dl, ln = lin
        _chk(dl, ln)
        unit = torch.empty(N, dtype=torch.float32, device=dev)
        _l.check(_lib().vqf_l2_norm_bwd_coef_lin(_ptr(dl), _ptr(ln), dl.shape[1], _ptr(norm), _ptr(inv), N, L, _ptr(cA),
                                                 _ptr(cB), _ptr(unit), _stream()), "vqf_l2_norm_bwd_coef_lin")
        return cA, cB, unit
    rowdot = torch.empty(N * L, dtype=torch.float32, device=dev)
    _l.check(_lib().vqf_rowdot(_ptr(Y), _ptr(dY), N * L, O, _ptr(rowdot), _stream()), "vqf_rowdot")
    _l.check(_lib().vqf_l2_norm_bwd_coef(_ptr(rowdot), _ptr(norm), _ptr(inv), N, L, _ptr(cA), _ptr(cB), _stream()),
             "vqf_l2_norm_bwd_coef")
    return cA, cB, inv


def _chk_roff(name, roff, U):
    """roff of the packed forms: a contiguous (U + 1,) int32 GPU tensor of row offsets (the kernels clamp what it holds)"""
    if not torch.is_tensor(roff) or not roff.is_cuda or roff.dtype != torch.int32 or not roff.is_contiguous() or \
            tuple(roff.shape) != (U + 1,):
        raise _l.VqfError("%s: roff must be a contiguous (%d,) int32 GPU tensor of row offsets" % (name, U + 1))


# The MFB fusion's launch entry points (include/vqa_fusion.h), every one of them, keyed by what selects it:
#   (direction, grouped, form, storage, rb)
#   direction  "fwd" | "bwd"
#   grouped    N questions over U shared images (idx; the backward also order / grp_off)
#   form       "plain": (N*L, 5*O) rows | "len": region counts (lens) | "packed": P holds the real rows (roff), Y (N*L, O) |
#              "rows": packed, and Y / dY on the real rows too (packed_coatt)
#   storage    "f32" | "pbf16": a bf16 P (and, in the backward, a bf16 dP) | "bf16dp": an fp32 P with a bf16 dP
#              ("pbf16_f32dp", a bf16 P with an fp32 dP, is the storage no entry has)
#   rb         the forward leaves the bf16 copy of R as well
# A key that is not here is a combination the library does not have: _fuse_entry says which rule it breaks.
_FUSE_ENTRIES = {
    ("fwd", False, "plain", "f32", False): "vqf_mfb_fuse_fwd",
    ("fwd", False, "plain", "pbf16", False): "vqf_mfb_fuse_fwd_pbf16",
    ("fwd", False, "plain", "pbf16", True): "vqf_mfb_fuse_fwd_pbf16_rb",
    ("fwd", False, "len", "f32", False): "vqf_mfb_fuse_fwd_len",
    ("fwd", False, "len", "pbf16", False): "vqf_mfb_fuse_fwd_len_pbf16",
    ("fwd", False, "len", "pbf16", True): "vqf_mfb_fuse_fwd_len_pbf16_rb",
    ("fwd", False, "packed", "f32", False): "vqf_mfb_fuse_fwd_packed",
    ("fwd", False, "packed", "pbf16", False): "vqf_mfb_fuse_fwd_packed_pbf16",
    ("fwd", False, "packed", "pbf16", True): "vqf_mfb_fuse_fwd_packed_pbf16_rb",
    ("fwd", False, "rows", "f32", False): "vqf_mfb_fuse_fwd_packed_rows",
    ("fwd", False, "rows", "pbf16", False): "vqf_mfb_fuse_fwd_packed_rows_pbf16",
    ("fwd", False, "rows", "pbf16", True): "vqf_mfb_fuse_fwd_packed_rows_pbf16_rb",
    ("fwd", True, "plain", "f32", False): "vqf_mfb_fuse_fwd_grouped",
    ("fwd", True, "len", "f32", False): "vqf_mfb_fuse_fwd_grouped_len",
    ("fwd", True, "packed", "f32", False): "vqf_mfb_fuse_fwd_grouped_packed",
    ("bwd", False, "plain", "f32", False): "vqf_mfb_fuse_bwd",
    ("bwd", False, "plain", "pbf16", False): "vqf_mfb_fuse_bwd_pbf16",
    ("bwd", False, "plain", "bf16dp", False): "vqf_mfb_fuse_bwd_bf16dp",
    ("bwd", False, "len", "f32", False): "vqf_mfb_fuse_bwd_len",
    ("bwd", False, "len", "pbf16", False): "vqf_mfb_fuse_bwd_len_pbf16",
    ("bwd", False, "len", "bf16dp", False): "vqf_mfb_fuse_bwd_len_bf16dp",
    ("bwd", False, "packed", "f32", False): "vqf_mfb_fuse_bwd_packed",
    ("bwd", False, "packed", "pbf16", False): "vqf_mfb_fuse_bwd_packed_pbf16",
    ("bwd", False, "packed", "bf16dp", False): "vqf_mfb_fuse_bwd_packed_bf16dp",
    ("bwd", False, "rows", "f32", False): "vqf_mfb_fuse_bwd_packed_rows",
    ("bwd", False, "rows", "pbf16", False): "vqf_mfb_fuse_bwd_packed_rows_pbf16",
    ("bwd", False, "rows", "bf16dp", False): "vqf_mfb_fuse_bwd_packed_rows_bf16dp",
    ("bwd", True, "plain", "f32", False): "vqf_mfb_fuse_bwd_grouped",
    ("bwd", True, "len", "f32", False): "vqf_mfb_fuse_bwd_grouped_len",
    ("bwd", True, "packed", "f32", False): "vqf_mfb_fuse_bwd_grouped_packed",
}
_FUSE_FULL = (False, "plain", "f32", False)        # the one pair of entries with cascade / zdrop / dzdrop / dcascade


def _fuse_entry(key, name="mfb_fuse"):
    """key -> the entry's name; a key outside _FUSE_ENTRIES is refused with the rule it breaks.  The rules the table states:
    a bf16 P comes with a bf16 dP; bf16 (P, dP, the copy of R) is un-grouped only; the copy of R is the forward's, beside a bf16 P;
    the packed rows are un-grouped."""
    entry = _FUSE_ENTRIES.get(key)
    if entry is not None:
        return entry
    direction, grouped, form, storage, rb = key
    if storage == "pbf16_f32dp":
        why = "a bf16 P comes with a bf16 dP"
    elif grouped and (storage != "f32" or rb):
        why = "a bf16 P / dP / r_bf16 is un-grouped only (the grouped fusion kernels are fp32; no idx / grp)"
    elif rb:
        why = "r_bf16 needs a bf16 P, normalise=False and no idx, in the forward"
    elif grouped and form == "rows":
        why = "Y on the packed rows is un-grouped only (no idx / grp)"
    else:
        why = "the library has no such entry"
    raise _l.VqfError("%s: %r: %s" % (name, key, why))


_FUSE_FORM_ARG = {"len": "lens", "packed": "roff", "rows": "roff (packed rows)"}


def _fuse_key(name, direction, grouped, form, P, dp_bf16=False, regions_bf16=False, rb=False, normalise=False, extras=False):
    """The key of a wrapper call into _FUSE_ENTRIES, refused here (before anything is allocated) where the call breaks a rule.
    Beside those of _fuse_entry, the rules the key does not hold:
    cascade / zdrop / dzdrop (extras) exist on the plain fp32 entry alone; on a layout form (lens / roff) bf16 needs regions_bf16
    (the models' attribute), and r_bf16 needs normalise=False."""
    if direction == "fwd":
        storage = "pbf16" if P.dtype == torch.bfloat16 else "f32"
    elif P.dtype == torch.bfloat16:
        storage = "pbf16" if dp_bf16 else "pbf16_f32dp"
    else:
        storage = "bf16dp" if dp_bf16 else "f32"
    if form != "plain":
        arg = _FUSE_FORM_ARG[form]
        if extras:
            raise _l.VqfError("%s: %s comes without cascade / zdrop / dzdrop" % (name, arg))
        if storage != "f32" and not regions_bf16:
            raise _l.VqfError("%s: %s takes an fp32 P / dP; bf16 ones with regions_bf16" % (name, arg))
        if rb and normalise:
            raise _l.VqfError("%s: %s: r_bf16 needs a bf16 P, normalise=False and no idx" % (name, arg))
    elif extras and storage != "f32":
        raise _l.VqfError("%s: a bf16 P / dP is only available without cascade / zdrop / dzdrop" % name)
    key = (direction, bool(grouped), form, storage, bool(rb))
    _fuse_entry(key, name)
    return key


def _fuse_fwd_args(key, P, pbias, q, keep, seed, p_drop, N, L, O, Rout, rowssq, stream, cascade=None, zdrop=None, idx=None, lens=(),
                   roff=None, U=None, R=None, R_bf16=None, ldrb=None, rb_rows=None):
    """key + operands (pointers or None, ints, floats; lens: the form's count pointers, (lens,) or (lens_q, lens_u))
    -> (entry name, its positional arguments in the header's order).  Pure."""
    entry = _fuse_entry(key)
    _, grouped, form, _, rb = key
    full, packed = key[1:] == _FUSE_FULL, form in ("packed", "rows")
    args = [P, pbias, q] + [cascade] * full + [idx] * grouped + list(lens) + [roff] * packed + [keep, seed, p_drop]
    args += [N] + [U] * grouped + [R] * packed + [L, O, Rout]
    if rb:
        args += [R_bf16, ldrb] + [rb_rows] * (form != "plain")
    return entry, tuple(args + [rowssq] + [zdrop] * full + [stream])


def _fuse_bwd_args(key, dY, Y, inv, coefA, coefB, P, pbias, q, keep, seed, p_drop, N, L, O, dP, dq, dbiasP, ws, ws_bytes, stream,
                   dzdrop=None, cascade=None, dcascade=None, idx=None, order=None, grp_off=None, lens=(), roff=None, U=None, R=None,
                   dP_rows=None):
    """_fuse_fwd_args for the backward entries"""
    entry = _fuse_entry(key)
    _, grouped, form, storage, _ = key
    full, packed = key[1:] == _FUSE_FULL, form in ("packed", "rows")
    args = [dY] + [dzdrop] * full + [Y, inv, coefA, coefB, P, pbias, q] + [cascade] * full + [idx, order, grp_off] * grouped
    args += list(lens) + [roff] * packed + [keep, seed, p_drop, N] + [U] * grouped + [R] * packed + [L, O, dP]
    args += [dP_rows] * (storage != "f32" and form != "plain") + [dq] + [dcascade] * full
    return entry, tuple(args + [dbiasP, ws, ws_bytes, stream])


def _fuse_fwd_run(key, P, pbias, q, keep, seed, p_drop, N, L, O, rows, r_bf16=None, rb_rows=0, cascade=None, zdrop=None, idx=None,
                  lens=(), roff=None, U=None, R=None):
    """The launch of every mfb_fuse_fwd* on the caller's stream, through _fuse_fwd_args (lens: a tuple of tensors)
    -> (the (rows, O) output, its four partial sums of squares per row, one per wave).  A key with rb: r_bf16 receives the
    (rb_rows, O rounded up to 32) bf16 copy, written whole by the call."""
    Rout = torch.empty((rows, O), dtype=torch.float32, device=P.device)
    rowssq = torch.empty(rows * 4, dtype=torch.float32, device=P.device)
    Rb = torch.empty((rb_rows, (O + 31) // 32 * 32), dtype=torch.bfloat16, device=P.device) if key[4] else None
    entry, args = _fuse_fwd_args(key, _ptr(P), _ptr(pbias), _ptr(q), _keep_ptr(keep), int(seed), float(p_drop), N, L, O, _ptr(Rout),
                                 _ptr(rowssq), _stream(), cascade=_ptr(cascade), zdrop=_ptr(zdrop), idx=_ptr(idx),
                                 lens=tuple(_ptr(x) for x in lens), roff=_ptr(roff), U=U, R=R, R_bf16=_ptr(Rb),
                                 ldrb=(O + 31) // 32 * 32, rb_rows=rb_rows)
    _l.check(getattr(_lib(), entry)(*args), entry)
    if Rb is not None:
        r_bf16.append(Rb)
    return Rout, rowssq


def _fuse_bwd_run(key, dY, Y, inv, cA, cB, P, pbias, q, keep, seed, p_drop, N, L, O, want_dbias, dp_rows, ws_bytes, dzdrop=None,
                  cascade=None, grp=None, lens=(), roff=None, U=None, R=None):
    """The launch of every mfb_fuse_bwd*, as _fuse_fwd_run; grp = (idx, order, grp_off) -> (dP, dq, dcascade or None, dbiasP or None).
    dP is like P, or -- a key with a bf16 dP -- bf16 with dp_rows rows: exact zeros behind the real ones on the region forms (the K
    padding of the weight gradient)."""
    dev = P.device
    idx, order, grp_off = (None, None, None) if grp is None else grp
    dq = torch.empty((N, POOL_K * O), dtype=torch.float32, device=dev)
    db = torch.empty(POOL_K * O, dtype=torch.float32, device=dev) if want_dbias else None
    dc = torch.empty_like(P) if cascade is not None else None
    dP = torch.empty_like(P) if key[3] == "f32" else torch.empty((dp_rows,) + tuple(P.shape[1:]), dtype=torch.bfloat16, device=dev)
    ws = workspace(dev, ws_bytes)
    entry, args = _fuse_bwd_args(key, _ptr(dY), _ptr(Y), _ptr(inv), _ptr(cA), _ptr(cB), _ptr(P), _ptr(pbias), _ptr(q), _keep_ptr(keep),
                                 int(seed), float(p_drop), N, L, O, _ptr(dP), _ptr(dq), _ptr(db), _ptr(ws), ws.numel(), _stream(),
                                 dzdrop=_ptr(dzdrop), cascade=_ptr(cascade), dcascade=_ptr(dc), idx=_ptr(idx), order=_ptr(order),
                                 grp_off=_ptr(grp_off), lens=tuple(_ptr(x) for x in lens), roff=_ptr(roff), U=U, R=R, dP_rows=dp_rows)
    _l.check(getattr(_lib(), entry)(*args), entry)
    return dP, dq, dc, db


def mfb_fuse_fwd(P, q, N, L, O, keep=None, seed=0, p_drop=0.0, cascade=None, want_zdrop=False, pbias=None,
                 normalise=True, r_bf16=None, lens=None, regions_bf16=False):
    """-> (Y normalised (N*L,O), norm (N), inv (N), zdrop or None).  pbias: projection bias added on load.
    P may be bf16 (written by gemm_bf16(out_bf16=True)), and then have more than N*L rows (the K padding of the weight gradient).
    normalise=False: the first output is R, the signed square roots WITHOUT the per-sample 1/norm (no vqf_scale_rows pass: the
    consumer applies inv in its GEMM epilogue).
    r_bf16: a list; it receives the bf16 copy of R with zero pad columns, written by the same launch (the operand of the consumer's
    bf16 GEMM): (N*L, O rounded up to 32), and QUIETLY nothing unless P is bf16, normalise=False and the padded O <= 1024.
    lens (N) int32: region counts -- sample n has lens[n] real rows (clamped to [1, L] in the kernel); the padded rows of P are not
    read, their rows of Y are exact zeros and norm runs over the real rows.  There r_bf16 has pad_rows(N*L) rows, zero behind each
    count and behind N*L.  What lens, bf16 and r_bf16 go with: _fuse_key."""
    (_chk_bf16 if P.dtype == torch.bfloat16 else _chk)(P)
    _chk(q, cascade, pbias)
    rb = r_bf16 is not None
    if lens is not None:
        _chk_lens(lens, N, "mfb_fuse_fwd")
    else:
        rb = rb and P.dtype == torch.bfloat16 and not normalise and (O + 31) // 32 * 32 <= 1024
    key = _fuse_key("mfb_fuse_fwd", "fwd", False, "plain" if lens is None else "len", P, regions_bf16=regions_bf16, rb=rb,
                    normalise=normalise, extras=cascade is not None or want_zdrop)
    zdrop = torch.empty_like(P) if want_zdrop else None
    R, rowssq = _fuse_fwd_run(key, P, pbias, q, keep, seed, p_drop, N, L, O, N * L, r_bf16, N * L if lens is None else pad_rows(N * L),
                              cascade=cascade, zdrop=zdrop, lens=() if lens is None else (lens,))
    return (R,) + _l2_norm_tail(R, rowssq, N, L, O, normalise) + (zdrop,)


def mfb_fuse_bwd(dY, Y, norm, inv, P, q, N, L, O, keep=None, seed=0, p_drop=0.0, cascade=None,
                 want_dbias=False, dzdrop=None, pbias=None, dp_bf16=False, lin=None, lens=None, dp_rows=None, regions_bf16=False):
    """-> (dP (N*L,5O) fp32 | bf16, dq (N,5O), dcascade or None, dbiasP or None).
    lin = (dlogits, lin) of the consumer's attention head: the UN-NORMALISED formulation -- Y is R (mfb_fuse_fwd(normalise=
    False)), dY is dYs = dY / norm, and sum(R * dYs) per sample comes from the head's (N*L, G) tensors instead of a
    rowdot pass over the (N*L, O) ones (vqf_l2_norm_bwd_coef_lin).
    dp_bf16: dP is bf16, shaped like P.
    lens (N) int32, with Y from mfb_fuse_fwd(lens=lens): dY / Y / P are not read on padded rows, whose dP rows are exact zeros; dq
    and dbiasP sum the real rows.  There a bf16 dP has dp_rows >= N*L rows (default: those of P, N*L at the least), exact zeros
    from row N*L on.  What lens and bf16 go with: _fuse_key."""
    (_chk_bf16 if P.dtype == torch.bfloat16 else _chk)(P)
    _chk(dY, Y, norm, inv, q, cascade, dzdrop, pbias)
    if lens is not None:
        _chk_lens(lens, N, "mfb_fuse_bwd")
    key = _fuse_key("mfb_fuse_bwd", "bwd", False, "plain" if lens is None else "len", P, dp_bf16=dp_bf16, regions_bf16=regions_bf16,
                    extras=cascade is not None or dzdrop is not None)
    cA, cB, inv = _l2_norm_bwd_coefs(dY, Y, norm, inv, N, L, O, lin)
    rows = P.shape[0] if lens is None else max(P.shape[0], N * L) if dp_rows is None else int(dp_rows)
    return _fuse_bwd_run(key, dY, Y, inv, cA, cB, P, pbias, q, keep, seed, p_drop, N, L, O, want_dbias, rows,
                         _lib().vqf_mfb_fuse_bwd_ws_bytes(N, L, O), dzdrop=dzdrop, cascade=cascade, lens=() if lens is None else (lens,))


def mfb_fuse_grouped_supported(N, U, L, O):
    return bool(_lib().vqf_mfb_fuse_grouped_supported(int(N), int(U), int(L), int(O)))


def _fuse_grouped_operands(name, P, q, N, U, L, O, pbias):
    _chk(P, q, pbias)
    if P.dim() != 2 or tuple(P.shape) != (U * L, POOL_K * O) or tuple(q.shape) != (N, POOL_K * O) or \
            (pbias is not None and tuple(pbias.shape) != (POOL_K * O,)):
        raise _l.VqfError("%s: P must be a contiguous (U*L, 5*O) = (%d, %d) tensor, q (N, 5*O) and pbias (5*O,); got P %s, q %s"
                          % (name, U * L, POOL_K * O, tuple(P.shape), tuple(q.shape)))
    if not mfb_fuse_grouped_supported(N, U, L, O):
        raise _l.VqfError("%s: N <= 65535, U <= 65535, O %% 4 == 0 and O <= 1024 are supported (got N=%d, U=%d, L=%d, O=%d)"
                          % (name, N, U, L, O))


def _chk_lens_grouped(name, lens, N, U):
    """lens of the grouped region-count forms: None -> (), or (lens_q (N,), lens_u (U,)), contiguous int32 GPU tensors"""
    if lens is None:
        return ()
    if not isinstance(lens, (tuple, list)) or len(lens) != 2:
        raise _l.VqfError(name + ": lens must be the pair (lens_q (N,), lens_u (U,))")
    _chk_lens(lens[0], N, name)
    _chk_lens(lens[1], U, name)
    return tuple(lens)


def mfb_fuse_fwd_grouped(P, q, idx, N, U, L, O, keep=None, seed=0, p_drop=0.0, pbias=None, normalise=True, lens=None):
    """The image fusion of N questions over U shared images: P (U*L, 5*O) fp32, q (N, 5*O), idx (N) int32 (question n reads the
    rows of image idx[n], clamped in the kernel); keep (N*L, 5*O) / the Philox draw stay per question
    -> (Y (N*L, O), norm (N), inv (N)) as mfb_fuse_fwd on P[idx] would give them, without that tensor.
    lens = (lens_q (N,), lens_u (U,)) int32: region counts per image and, gathered, per question (mfb_fuse_fwd's lens)."""
    _fuse_grouped_operands("mfb_fuse_fwd_grouped", P, q, N, U, L, O, pbias)
    _chk_group("mfb_fuse_fwd_grouped", N, U, idx=idx)
    lens = _chk_lens_grouped("mfb_fuse_fwd_grouped", lens, N, U)
    key = _fuse_key("mfb_fuse_fwd_grouped", "fwd", True, "len" if lens else "plain", P)
    R, rowssq = _fuse_fwd_run(key, P, pbias, q, keep, seed, p_drop, N, L, O, N * L, idx=idx, U=U, lens=lens)
    return (R,) + _l2_norm_tail(R, rowssq, N, L, O, normalise)


def mfb_fuse_bwd_grouped(dY, Y, norm, inv, P, q, idx, order, grp_off, N, U, L, O, keep=None, seed=0, p_drop=0.0,
                         want_dbias=False, pbias=None, lin=None, lens=None):
    """-> (dP (U*L, 5*O): the sum over each image's questions, added in `order` (zero rows for an image without a question),
    dq (N, 5*O), dbiasP or None).  lin as in mfb_fuse_bwd.  No (N*L, 5*O) tensor is allocated.
    lens = (lens_q, lens_u) as in mfb_fuse_fwd_grouped: the dP rows beyond an image's count are exact zeros."""
    _fuse_grouped_operands("mfb_fuse_bwd_grouped", P, q, N, U, L, O, pbias)
    _chk_group("mfb_fuse_bwd_grouped", N, U, idx=idx, order=order, grp_off=grp_off)
    lens = _chk_lens_grouped("mfb_fuse_bwd_grouped", lens, N, U)
    _chk(dY, Y, norm, inv)
    if tuple(dY.shape) != (N * L, O) or tuple(Y.shape) != (N * L, O):
        raise _l.VqfError("mfb_fuse_bwd_grouped: dY and Y must be (N*L, O)")
    key = _fuse_key("mfb_fuse_bwd_grouped", "bwd", True, "len" if lens else "plain", P)
    cA, cB, inv = _l2_norm_bwd_coefs(dY, Y, norm, inv, N, L, O, lin)
    dP, dq, _, db = _fuse_bwd_run(key, dY, Y, inv, cA, cB, P, pbias, q, keep, seed, p_drop, N, L, O, want_dbias, None,
                                  _lib().vqf_mfb_fuse_bwd_grouped_ws_bytes(N, U, L, O), grp=(idx, order, grp_off), U=U, lens=lens)
    return dP, dq, db


# the packed forms (include/vqa_fusion.h "Packed region features"): P / dP / the pooled features hold the real rows of every image, one
# image after the other; roff = int32 row offsets, (N + 1) per sample or -- with idx -- (U + 1) per image.  The kernels clamp what
# roff holds; only its type, shape and device are checked here.
def mfb_fuse_packed_supported(N, U, R, L, O):
    return bool(_lib().vqf_mfb_fuse_packed_supported(int(N), int(U), int(R), int(L), int(O)))


def _packed_operands(name, P, q, roff, N, U, L, O, pbias, R=None, regions_bf16=False):
    """-> R, the real rows of P: P.shape[0], or the R given where P (bf16) has more rows behind them (the K padding of the weight
    gradient).  regions_bf16: a bf16 P is taken (the un-grouped forms' vqf_mfb_fuse_*_packed*_pbf16)."""
    if regions_bf16 and P.dtype == torch.bfloat16:
        _chk_bf16(P)
        if not P.is_contiguous():
            raise _l.VqfError(name + ": contiguous tensor expected")
    else:
        _chk(P)
    _chk(q, pbias)
    R = (P.shape[0] if P.dim() == 2 else 0) if R is None else int(R)
    if P.dim() != 2 or R < 1 or R > P.shape[0] or P.shape[1] != POOL_K * O or tuple(q.shape) != (N, POOL_K * O) or \
            (pbias is not None and tuple(pbias.shape) != (POOL_K * O,)):
        raise _l.VqfError("%s: P must be a contiguous (R, 5*O) tensor with R >= 1, q (N, 5*O) and pbias (5*O,); got P %s, q %s"
                          % (name, tuple(P.shape), tuple(q.shape)))
    _chk_roff(name, roff, U)
    if not mfb_fuse_packed_supported(N, U, R, L, O):
        raise _l.VqfError("%s: N <= 65535, U <= 65535, L <= 1024, O %% 4 == 0 and O <= 1024 are supported (got N=%d, U=%d, R=%d, "
                          "L=%d, O=%d)" % (name, N, U, R, L, O))
    return R


def mfb_fuse_fwd_packed(P, q, roff, N, L, O, idx=None, keep=None, seed=0, p_drop=0.0, pbias=None, normalise=True, R=None,
                        regions_bf16=False, r_bf16=None):
    """The image fusion on packed rows: P (R, 5*O) fp32, q (N, 5*O), roff (N + 1) int32 -- with idx (N) int32: (U + 1), question n
    reads the rows of image idx[n]; keep (N*L, 5*O) / the Philox draw stay in the padded coordinates
    -> (Y (N*L, O), norm (N), inv (N)): the bits of mfb_fuse_fwd(lens=) / mfb_fuse_fwd_grouped(lens=) on the zero-padded copy of P.
    A bf16 P may hold more than the R real rows given.  r_bf16 (a list) receives the (pad_rows(N*L), O rounded up to 32) bf16 copy
    of Y the same launch wrote, zero rows behind each count and behind N*L.  What bf16 and r_bf16 go with: _fuse_key."""
    U = N if idx is None else roff.shape[0] - 1
    key = _fuse_key("mfb_fuse_fwd_packed", "fwd", idx is not None, "packed", P, regions_bf16=regions_bf16, rb=r_bf16 is not None,
                    normalise=normalise)
    R = _packed_operands("mfb_fuse_fwd_packed", P, q, roff, N, U, L, O, pbias, R, regions_bf16)
    if idx is not None:
        _chk_group("mfb_fuse_fwd_packed", N, U, idx=idx)
    Y, rowssq = _fuse_fwd_run(key, P, pbias, q, keep, seed, p_drop, N, L, O, N * L, r_bf16, pad_rows(N * L), idx=idx, roff=roff, U=U, R=R)
    return (Y,) + _l2_norm_tail(Y, rowssq, N, L, O, normalise)


def mfb_fuse_bwd_packed(dY, Y, norm, inv, P, q, roff, N, L, O, grp=None, keep=None, seed=0, p_drop=0.0, want_dbias=False, pbias=None,
                        lin=None, dp_bf16=False, R=None, dp_rows=None, regions_bf16=False):
    """-> (dP (R, 5*O), dq (N, 5*O), dbiasP or None).  grp = (idx, order, grp_off): roff is per image and dP sums each image's
    questions in `order` (zero rows for an image without a question).  lin as in mfb_fuse_bwd.
    dp_bf16 (P fp32 or bf16, of which R rows are real): dP is bf16 with dp_rows >= R rows (default: those of P), exact zeros from
    row R on -- the K padding of the weight gradient.  What bf16 goes with: _fuse_key."""
    U = N if grp is None else roff.shape[0] - 1
    key = _fuse_key("mfb_fuse_bwd_packed", "bwd", grp is not None, "packed", P, dp_bf16=dp_bf16, regions_bf16=regions_bf16)
    R = _packed_operands("mfb_fuse_bwd_packed", P, q, roff, N, U, L, O, pbias, R, regions_bf16)
    _chk(dY, Y, norm, inv)
    if tuple(dY.shape) != (N * L, O) or tuple(Y.shape) != (N * L, O):
        raise _l.VqfError("mfb_fuse_bwd_packed: dY and Y must be (N*L, O)")
    if grp is not None:
        _chk_group("mfb_fuse_bwd_packed", N, U, idx=grp[0], order=grp[1], grp_off=grp[2])
    cA, cB, inv = _l2_norm_bwd_coefs(dY, Y, norm, inv, N, L, O, lin)
    ws_bytes = _lib().vqf_mfb_fuse_bwd_ws_bytes(N, L, O) if grp is None else _lib().vqf_mfb_fuse_bwd_grouped_ws_bytes(N, U, L, O)
    dP, dq, _, db = _fuse_bwd_run(key, dY, Y, inv, cA, cB, P, pbias, q, keep, seed, p_drop, N, L, O, want_dbias,
                                  P.shape[0] if dp_rows is None else int(dp_rows), ws_bytes, grp=grp, roff=roff, U=U, R=R)
    return dP, dq, db


def _pool_packed_dims(name, feat, roff, logits_or_wts_G, N, S, idx):
    _chk(feat)
    if feat.dim() != 2 or feat.shape[0] < 1:
        raise _l.VqfError(name + ": feat must be a contiguous (R, C) fp32 GPU tensor with R >= 1")
    R, C = feat.shape
    U = N if idx is None else roff.shape[0] - 1
    _chk_roff(name, roff, U)
    if idx is not None:
        _chk_group(name, N, U, idx=idx)
    if not glimpse_pool_grouped_supported(N, U, S, C, logits_or_wts_G):
        raise _l.VqfError(name + ": N <= 65535, U <= 65535, S <= 1024, C %% 4 == 0 and G in {1, 2, 3} are supported "
                          "(got N=%d, U=%d, S=%d, C=%d, G=%d)" % (N, U, S, C, logits_or_wts_G))
    return U, R, C


def glimpse_pool_fwd_packed(feat, logits, roff, N, S, unit_softmax, idx=None):
    """feat (R, C) packed rows, logits (N*S, G), roff (N + 1) int32 -- with idx (N) int32: (U + 1) per image
    -> wts (N, G, S) (exact zeros beyond the count), pooled (N, G*C): glimpse_pool_fwd(lens=) / _grouped(lens=) on the padded copy."""
    _chk(logits)
    G = logits.shape[1]
    U, R, C = _pool_packed_dims("glimpse_pool_fwd_packed", feat, roff, G, N, S, idx)
    if logits.shape[0] != N * S:
        raise _l.VqfError("glimpse_pool_fwd_packed: logits must be (N*S, G)")
    wts = torch.empty((N, G, S), dtype=torch.float32, device=feat.device)
    pooled = torch.empty((N, G * C), dtype=torch.float32, device=feat.device)
    _l.check(_lib().vqf_glimpse_pool_fwd_packed(_ptr(feat), _ptr(logits), _ptr(idx), _ptr(roff), N, U, R, S, C, G,
                                                int(bool(unit_softmax)), _ptr(wts), _ptr(pooled), _stream()),
             "vqf_glimpse_pool_fwd_packed")
    return wts, pooled


def glimpse_pool_bwd_packed(dpooled, feat, wts, roff, unit_softmax, idx=None, dwts=None):
    """dpooled (N, G*C), feat (R, C) data, wts (N, G, S) -> dlogits (N*S, G), exact zeros beyond the count"""
    _chk(dpooled, wts, dwts)
    N, G, S = wts.shape
    U, R, C = _pool_packed_dims("glimpse_pool_bwd_packed", feat, roff, G, N, S, idx)
    if tuple(dpooled.shape) != (N, G * C) or (dwts is not None and tuple(dwts.shape) != (N, G, S)):
        raise _l.VqfError("glimpse_pool_bwd_packed: dpooled must be (N, G*C), wts and dwts (N, G, S)")
    dlogits = torch.empty((N * S, G), dtype=torch.float32, device=feat.device)
    _l.check(_lib().vqf_glimpse_pool_bwd_packed(_ptr(dpooled), _ptr(dwts), _ptr(feat), _ptr(wts), _ptr(idx), _ptr(roff), N, U, R, S, C,
                                                G, int(bool(unit_softmax)), _ptr(dlogits), _stream()), "vqf_glimpse_pool_bwd_packed")
    return dlogits


def glimpse_pool_bwd_packed_dfeat(dpooled, feat, wts, roff, unit_softmax, grp=None, dwts=None):
    """glimpse_pool_bwd_packed with the gradient of the packed rows: -> (dlogits (N*S, G), dfeat (R, C)).  grp None: sample n owns
    roff[n] ..; grp = (idx, order, grp_off): roff is per image and dfeat sums each image's questions in `order` (zeros for an image
    without a question).  glimpse_pool_bwd(lens=) / _grouped(lens=) on the padded copy, dfeat its real rows."""
    _chk(dpooled, wts, dwts)
    N, G, S = wts.shape
    idx, order, grp_off = grp if grp is not None else (None, None, None)
    U, R, C = _pool_packed_dims("glimpse_pool_bwd_packed_dfeat", feat, roff, G, N, S, idx)
    if grp is not None:
        _chk_group("glimpse_pool_bwd_packed_dfeat", N, U, order=order, grp_off=grp_off)
    if tuple(dpooled.shape) != (N, G * C) or (dwts is not None and tuple(dwts.shape) != (N, G, S)):
        raise _l.VqfError("glimpse_pool_bwd_packed_dfeat: dpooled must be (N, G*C), wts and dwts (N, G, S)")
    dlogits = torch.empty((N * S, G), dtype=torch.float32, device=feat.device)
    dfeat = torch.empty_like(feat)
    _l.check(_lib().vqf_glimpse_pool_bwd_packed_dfeat(_ptr(dpooled), _ptr(dwts), _ptr(feat), _ptr(wts), _ptr(idx), _ptr(order),
                                                      _ptr(grp_off), _ptr(roff), N, U, R, S, C, G, int(bool(unit_softmax)),
                                                      _ptr(dlogits), _ptr(dfeat), _stream()), "vqf_glimpse_pool_bwd_packed_dfeat")
    return dlogits, dfeat


# the co-attention head on the packed rows (include/vqa_fusion.h "The co-attention head on the packed rows"; MFB / MHBCoAtt
# packed_coatt): the fusion's output, its gradient, rowssq, the logits and their gradient hold the R real rows as well.  Un-grouped.
def l2_group_norm_packed(rowssq, roff, N, R, L):
    """rowssq (4*R) packed partials -> (norm (N), inv (N), rowinv (R) = inv of each row's owner)"""
    _chk(rowssq)
    _chk_roff("l2_group_norm_packed", roff, N)
    if rowssq.numel() != 4 * R:
        raise _l.VqfError("l2_group_norm_packed: rowssq must hold 4*R = %d partials, got %d" % (4 * R, rowssq.numel()))
    dev = rowssq.device
    norm = torch.empty(N, dtype=torch.float32, device=dev)
    inv = torch.empty(N, dtype=torch.float32, device=dev)
    rowinv = torch.empty(R, dtype=torch.float32, device=dev)
    _l.check(_lib().vqf_l2_group_norm_packed(_ptr(rowssq), _ptr(roff), N, R, L, _ptr(norm), _ptr(inv), _ptr(rowinv), _stream()),
             "vqf_l2_group_norm_packed")
    return norm, inv, rowinv


def l2_norm_bwd_coef_packed(rowdot, roff, norm, inv, N, L):
    """rowdot (R) packed -> (coefA (N), coefB (N)) of vqf_l2_norm_bwd_coef"""
    _chk(rowdot, norm, inv)
    _chk_roff("l2_norm_bwd_coef_packed", roff, N)
    if tuple(norm.shape) != (N,) or tuple(inv.shape) != (N,) or rowdot.dim() != 1:
        raise _l.VqfError("l2_norm_bwd_coef_packed: rowdot must be (R,), norm and inv (N,)")
    cA = torch.empty(N, dtype=torch.float32, device=rowdot.device)
    cB = torch.empty(N, dtype=torch.float32, device=rowdot.device)
    _l.check(_lib().vqf_l2_norm_bwd_coef_packed(_ptr(rowdot), _ptr(roff), _ptr(norm), _ptr(inv), N, rowdot.shape[0], L, _ptr(cA),
                                                _ptr(cB), _stream()), "vqf_l2_norm_bwd_coef_packed")
    return cA, cB


def l2_norm_bwd_coef_lin_packed(dlogits, lin, roff, norm, inv, N, L):
    """dlogits, lin (R, G) packed -> (coefA (N), coefB (N), unit (N)) of vqf_l2_norm_bwd_coef_lin"""
    _chk(dlogits, lin, norm, inv)
    _chk_roff("l2_norm_bwd_coef_lin_packed", roff, N)
    if dlogits.dim() != 2 or dlogits.shape != lin.shape or tuple(norm.shape) != (N,) or tuple(inv.shape) != (N,):
        raise _l.VqfError("l2_norm_bwd_coef_lin_packed: dlogits and lin must be (R, G), norm and inv (N,)")
    dev = dlogits.device
    cA = torch.empty(N, dtype=torch.float32, device=dev)
    cB = torch.empty(N, dtype=torch.float32, device=dev)
    unit = torch.empty(N, dtype=torch.float32, device=dev)
    _l.check(_lib().vqf_l2_norm_bwd_coef_lin_packed(_ptr(dlogits), _ptr(lin), dlogits.shape[1], _ptr(roff), _ptr(norm), _ptr(inv), N,
                                                    dlogits.shape[0], L, _ptr(cA), _ptr(cB), _ptr(unit), _stream()),
             "vqf_l2_norm_bwd_coef_lin_packed")
    return cA, cB, unit


def mfb_fuse_fwd_packed_rows(P, q, roff, N, L, O, keep=None, seed=0, p_drop=0.0, pbias=None, normalise=True, R=None,
                             regions_bf16=False, r_bf16=None):
    """mfb_fuse_fwd_packed with the output on the packed rows: P (R, 5*O), q (N, 5*O), roff (N + 1) int32; keep (N*L, 5*O) / the Philox
    draw stay in the padded coordinates -> (Y (R, O), norm (N), inv (N), rowinv (R)): the real rows of mfb_fuse_fwd_packed's Y, bit
    for bit; nothing of N*L rows is allocated.  rowinv[r] = inv of row r's sample (the consumers' per-row scale).
    r_bf16 as there, with pad_rows(R) rows: zero rows behind R."""
    key = _fuse_key("mfb_fuse_fwd_packed_rows", "fwd", False, "rows", P, regions_bf16=regions_bf16, rb=r_bf16 is not None,
                    normalise=normalise)
    R = _packed_operands("mfb_fuse_fwd_packed_rows", P, q, roff, N, N, L, O, pbias, R, regions_bf16)
    Y, rowssq = _fuse_fwd_run(key, P, pbias, q, keep, seed, p_drop, N, L, O, R, r_bf16, pad_rows(R), roff=roff, R=R)
    norm, inv, rowinv = l2_group_norm_packed(rowssq, roff, N, R, L)
    if normalise:
        _l.check(_lib().vqf_scale_rows(_ptr(Y), _ptr(rowinv), R, 1, O, _ptr(Y), _stream()), "vqf_scale_rows")
    return Y, norm, inv, rowinv


def mfb_fuse_bwd_packed_rows(dY, Y, norm, inv, P, q, roff, N, L, O, keep=None, seed=0, p_drop=0.0, want_dbias=False, pbias=None,
                             lin=None, dp_bf16=False, R=None, dp_rows=None, regions_bf16=False):
    """mfb_fuse_bwd_packed with dY / Y (R, O) on the packed rows (and lin = (dlogits, lin) (R, G)) -> (dP (R, 5*O), dq (N, 5*O),
    dbiasP or None); dp_bf16 / R / dp_rows as there."""
    key = _fuse_key("mfb_fuse_bwd_packed_rows", "bwd", False, "rows", P, dp_bf16=dp_bf16, regions_bf16=regions_bf16)
    R = _packed_operands("mfb_fuse_bwd_packed_rows", P, q, roff, N, N, L, O, pbias, R, regions_bf16)
    _chk(dY, Y, norm, inv)
    if tuple(dY.shape) != (R, O) or tuple(Y.shape) != (R, O):
        raise _l.VqfError("mfb_fuse_bwd_packed_rows: dY and Y must be (R, O) = (%d, %d)" % (R, O))
    if lin is not None:
        cA, cB, inv = l2_norm_bwd_coef_lin_packed(lin[0], lin[1], roff, norm, inv, N, L)
    else:
        rowdot = torch.empty(R, dtype=torch.float32, device=P.device)
        _l.check(_lib().vqf_rowdot(_ptr(Y), _ptr(dY), R, O, _ptr(rowdot), _stream()), "vqf_rowdot")
        cA, cB = l2_norm_bwd_coef_packed(rowdot, roff, norm, inv, N, L)
    dP, dq, _, db = _fuse_bwd_run(key, dY, Y, inv, cA, cB, P, pbias, q, keep, seed, p_drop, N, L, O, want_dbias,
                                  P.shape[0] if dp_rows is None else int(dp_rows), _lib().vqf_mfb_fuse_bwd_ws_bytes(N, L, O), roff=roff,
                                  R=R)
    return dP, dq, db


def glimpse_pool_fwd_packed_rows(feat, logits, roff, N, S, unit_softmax):
    """glimpse_pool_fwd_packed with logits (R, G) on the packed rows -> wts (N, G, S) (exact zeros beyond the count), pooled (N, G*C)"""
    _chk(logits)
    G = logits.shape[1]
    U, R, C = _pool_packed_dims("glimpse_pool_fwd_packed_rows", feat, roff, G, N, S, None)
    if logits.shape[0] != R:
        raise _l.VqfError("glimpse_pool_fwd_packed_rows: logits must be (R, G) = (%d, %d)" % (R, G))
    wts = torch.empty((N, G, S), dtype=torch.float32, device=feat.device)
    pooled = torch.empty((N, G * C), dtype=torch.float32, device=feat.device)
    _l.check(_lib().vqf_glimpse_pool_fwd_packed_rows(_ptr(feat), _ptr(logits), None, _ptr(roff), N, U, R, S, C, G,
                                                     int(bool(unit_softmax)), _ptr(wts), _ptr(pooled), _stream()),
             "vqf_glimpse_pool_fwd_packed_rows")
    return wts, pooled


def glimpse_pool_bwd_packed_rows(dpooled, feat, wts, roff, unit_softmax, dwts=None):
    """dpooled (N, G*C), feat (R, C) data, wts (N, G, S) -> dlogits (R, G) on the packed rows"""
    _chk(dpooled, wts, dwts)
    N, G, S = wts.shape
    U, R, C = _pool_packed_dims("glimpse_pool_bwd_packed_rows", feat, roff, G, N, S, None)
    if tuple(dpooled.shape) != (N, G * C) or (dwts is not None and tuple(dwts.shape) != (N, G, S)):
        raise _l.VqfError("glimpse_pool_bwd_packed_rows: dpooled must be (N, G*C), wts and dwts (N, G, S)")
    dlogits = torch.empty((R, G), dtype=torch.float32, device=feat.device)
    _l.check(_lib().vqf_glimpse_pool_bwd_packed_rows(_ptr(dpooled), _ptr(dwts), _ptr(feat), _ptr(wts), None, _ptr(roff), N, U, R, S, C,
                                                     G, int(bool(unit_softmax)), _ptr(dlogits), _stream()),
             "vqf_glimpse_pool_bwd_packed_rows")
    return dlogits


# the packed forms of the guided attention logits: xh / dxh (R, G*E) hold the real rows only (include/vqa_fusion.h "The packed forms
# of the alternating image side").  The kernels clamp what roff and the index arrays hold; only type, shape and device are checked here.
def guided_logits_packed_supported(N, U, R, S, E, G):
    return bool(_lib().vqf_guided_logits_packed_supported(int(N), int(U), int(R), int(S), int(E), int(G)))


def _guided_packed_operands(name, xh, gp, w, roff, N, S, grouped):
    _chk2s(xh)
    _chk(gp, w)
    G, E = w.shape
    if xh.dim() != 2 or xh.shape[0] < 1 or xh.shape[1] != G * E or (gp is not None and tuple(gp.shape) != (N, G * E)):
        raise _l.VqfError(name + ": xh must be (R, G*E) with R >= 1, gp (N, G*E) or None, w (G, E)")
    R = xh.shape[0]
    U = roff.shape[0] - 1 if grouped and torch.is_tensor(roff) else N
    _chk_roff(name, roff, U)
    if not guided_logits_packed_supported(N, U, R, S, E, G):
        raise _l.VqfError(name + ": E %% 32 == 0, E <= 1024, 1 <= S <= 1024, G in {1, 2, 3}, N <= 65535, U <= 65535 and "
                          "1 <= R < 2^29 are supported (got N=%d, U=%d, R=%d, S=%d, E=%d, G=%d)" % (N, U, R, S, E, G))
    return G, E, U, R


def guided_logits_fwd_packed(xh, gp, w, roff, N, S, idx=None):
    """xh (R, G*E) packed rows (rows may be strided), gp (N, G*E) or None, w (G, E), roff (N + 1) int32 -- with idx (N) int32:
    (U + 1) per image -> logits (N*S, G): guided_logits_fwd / _grouped on the padded copy, exact zeros behind each count."""
    G, E, U, R = _guided_packed_operands("guided_logits_fwd_packed", xh, gp, w, roff, N, S, idx is not None)
    if idx is not None:
        _chk_group("guided_logits_fwd_packed", N, U, idx=idx)
    out = torch.empty((N * S, G), dtype=torch.float32, device=xh.device)
    _l.check(_lib().vqf_guided_logits_fwd_packed(_ptr(xh), xh.stride(0), _ptr(gp), _ptr(w), _ptr(idx), _ptr(roff), int(N), U, R, int(S),
                                                 E, G, _ptr(out), _stream()), "vqf_guided_logits_fwd_packed")
    return out


def guided_logits_bwd_packed(dlogits, xh, gp, w, roff, N, S, grp=None, out=None):
    """-> (dxh (R, G*E) packed (out: written there, rows may be strided), dgp (N, G*E), dw (G, E)).  grp None: sample n owns
    roff[n] ..; grp = (idx, order, grp_off): dxh sums each image's questions in `order` (zero rows for an image without a question).
    dgp and dw are summed in the order of guided_logits_bwd / _grouped on the padded copy; dlogits rows behind a count are not read."""
    G, E, U, R = _guided_packed_operands("guided_logits_bwd_packed", xh, gp, w, roff, N, S, grp is not None)
    order, grp_off = (grp[1], grp[2]) if grp is not None else (None, None)
    if grp is not None:
        _chk_group("guided_logits_bwd_packed", N, U, order=order, grp_off=grp_off)
        if gp is None:
            raise _l.VqfError("guided_logits_bwd_packed: the grouped form needs gp (N, G*E)")
    _chk(dlogits)
    _chk2s(out)
    if tuple(dlogits.shape) != (N * S, G) or (out is not None and tuple(out.shape) != (R, G * E)):
        raise _l.VqfError("guided_logits_bwd_packed: dlogits must be (N*S, G) and out (R, G*E)")
    if out is None:
        out = torch.empty((R, G * E), dtype=torch.float32, device=xh.device)
    dgp = torch.empty((N, G * E), dtype=torch.float32, device=xh.device)
    dw = torch.empty((G, E), dtype=torch.float32, device=xh.device)
    ws = workspace(xh.device, _lib().vqf_guided_logits_bwd_packed_ws_bytes(int(N), U, int(S), E, G))
    _l.check(_lib().vqf_guided_logits_bwd_packed(_ptr(dlogits), _ptr(xh), xh.stride(0), _ptr(gp), _ptr(w), _ptr(order), _ptr(grp_off),
                                                 _ptr(roff), int(N), U, R, int(S), E, G, _ptr(out), out.stride(0), _ptr(dgp), _ptr(dw),
                                                 _ptr(ws), ws.numel(), _stream()), "vqf_guided_logits_bwd_packed")
    return out, dgp, dw


def lstm_seq_supported(B, H):
    return bool(_lib().vqf_lstm_seq_supported(int(B), int(H)))


def _lstm_seq_ws(B, H, device):
    nbytes = int(_lib().vqf_lstm_seq_ws_bytes(int(B), int(H)))
    return workspace(device, nbytes), nbytes


def lstm_seq_fwd(xw, w_hh, bf16=False):
    """xw (S,B,4H) = x W_ih^T + biases, w_hh (4H,H) -> hs (S,B,H), cs (S,B,H), gates (S,B,4H) activated.
    bf16: the recurrent product takes bf16 operands (fp32 accumulate; bf16 mode)."""
    _chk(xw, w_hh)
    S, B, H4 = xw.shape
    H = H4 // 4
    hs = torch.empty((S, B, H), dtype=torch.float32, device=xw.device)
    cs = torch.empty_like(hs)
    gates = torch.empty_like(xw)
    ws, nb = _lstm_seq_ws(B, H, xw.device)
    _l.check(_lib().vqf_lstm_seq_fwd(_ptr(xw), _ptr(w_hh), S, B, H, _ptr(hs), _ptr(cs), _ptr(gates),
                                     1 if bf16 else 0, _ptr(ws), nb, _stream()), "vqf_lstm_seq_fwd")
    return hs, cs, gates


def lstm_seq_bwd(dhs, gates, cs, w_hh, bf16=False):
    """-> dgates (S,B,4H): gradient w.r.t. the gate pre-activations; w_hh (4H,H) as stored."""
    _chk(dhs, gates, cs, w_hh)
    S, B, H = dhs.shape
    dgates = torch.empty_like(gates)
    carry = torch.empty((B, H), dtype=torch.float32, device=dhs.device)
    ws, nb = _lstm_seq_ws(B, H, dhs.device)
    _l.check(_lib().vqf_lstm_seq_bwd(_ptr(dhs), _ptr(gates), _ptr(cs), _ptr(w_hh), S, B, H, _ptr(dgates),
                                     _ptr(carry), 1 if bf16 else 0, _ptr(ws), nb, _stream()), "vqf_lstm_seq_bwd")
    return dgates


def lstm_cell_fwd(gates, c_prev, c_out, h_out):
    """gates (B,4H) pre-activations -> activated in place; writes c_out, h_out (B,H)."""
    _chk(gates, c_prev, c_out, h_out)
    B, H4 = gates.shape
    _l.check(_lib().vqf_lstm_cell_fwd(_ptr(gates), _ptr(c_prev), B, H4 // 4, _ptr(c_out), _ptr(h_out), _stream()),
             "vqf_lstm_cell_fwd")


def lstm_step_supported(B, H):
    return bool(_lib().vqf_lstm_step_supported(int(B), int(H)))


def lstm_step_fwd(h_prev, w_hh, gates, c_prev, c_out, h_out):
    """one LSTM step in one launch: gates (B,4H) += h_prev W_hh^T, then the cell in the product's epilogue (include/vqa_fusion.h)"""
    _chk(h_prev, w_hh, gates, c_prev, c_out, h_out)
    B, H4 = gates.shape
    _l.check(_lib().vqf_lstm_step_fwd(_ptr(h_prev), _ptr(w_hh), _ptr(gates), _ptr(c_prev), B, H4 // 4, _ptr(c_out), _ptr(h_out),
                                      _stream()), "vqf_lstm_step_fwd")


def lstm_cell_bwd(dhs_t, dh_carry, gates, c_t, c_prev, first, dc_carry, dG):
    _chk(dhs_t, dh_carry, gates, c_t, c_prev, dc_carry, dG)
    B, H = dhs_t.shape
    _l.check(_lib().vqf_lstm_cell_bwd(_ptr(dhs_t), _ptr(dh_carry), _ptr(gates), _ptr(c_t), _ptr(c_prev), int(bool(first)),
                                      B, H, _ptr(dc_carry), _ptr(dG), _stream()), "vqf_lstm_cell_bwd")


# ---------------------------------------------------------------------------
# question-encoder front end (mfb.py:68)
def _chk_ids(ids):
    if not ids.is_cuda or ids.dtype != torch.int64 or not ids.is_contiguous():
        raise _l.VqfError("contiguous int64 GPU token ids expected")


def embed_tanh_fwd(weight, ids, tanh=True, time_major=False, lens=None):
    """tanh(weight[ids]) (tanh=False: weight[ids]): weight (V,E) fp32, ids any shape int64 -> ids.shape + (E,);
    time_major (ids (N,Tq), tanh only): -> (Tq, N, E), the rows in the order the batch-major LSTM walks them;
    lens (N) int32 (ids (N,Tq), tanh, sample-major): the rows of the tokens at positions >= lens[n] are zero"""
    _chk(weight)
    _chk_ids(ids)
    V, E = weight.shape
    T = ids.numel()
    if lens is not None:
        if not tanh or time_major or ids.dim() != 2:
            raise _l.VqfError("embed_tanh_fwd: lens goes with (N, Tq) ids, tanh and sample-major rows")
        N, Tq = ids.shape
        _chk_lens(lens, N, "embed_tanh_fwd")
        out = torch.empty((N, Tq, E), dtype=torch.float32, device=weight.device)
        _l.check(_lib().vqf_embed_tanh_fwd_len(_ptr(weight), ctypes.c_void_p(ids.data_ptr()), _ptr(lens), N, Tq, V, E, _ptr(out),
                                               _stream()), "vqf_embed_tanh_fwd_len")
        return out
    if time_major:
        if not tanh or ids.dim() != 2:
            raise _l.VqfError("embed_tanh_fwd: the time-major form takes (N, Tq) ids and applies tanh")
        N, Tq = ids.shape
        out = torch.empty((Tq, N, E), dtype=torch.float32, device=weight.device)
        _l.check(_lib().vqf_embed_tanh_fwd_tm(_ptr(weight), ctypes.c_void_p(ids.data_ptr()), N, Tq, V, E, _ptr(out), _stream()),
                 "vqf_embed_tanh_fwd_tm")
        return out
    out = torch.empty(tuple(ids.shape) + (E,), dtype=torch.float32, device=weight.device)
    fn = _lib().vqf_embed_tanh_fwd if tanh else _lib().vqf_embed_fwd
    _l.check(fn(_ptr(weight), ctypes.c_void_p(ids.data_ptr()), T, V, E, _ptr(out), _stream()), "vqf_embed_fwd")
    return out


def embed_dropout_fwd(weight, ids, keep=None, seed=0, p_drop=0.5):
    """dropout(weight[ids]) in one launch: -> (ids.numel(), E); the mask of ops.dropout over that flat tensor"""
    _chk(weight)
    _chk_ids(ids)
    V, E = weight.shape
    out = torch.empty((ids.numel(), E), dtype=torch.float32, device=weight.device)
    _l.check(_lib().vqf_embed_dropout_fwd(_ptr(weight), ctypes.c_void_p(ids.data_ptr()), ids.numel(), V, E, _keep_ptr(keep), int(seed),
                                          float(p_drop), _ptr(out), _stream()), "vqf_embed_dropout_fwd")
    return out


def embed_dropout_bwd(dout, ids, V, keep=None, seed=0, p_drop=0.5):
    """-> dW (V, E) = segment sums of dout * keep / (1 - p) over the tokens of each id, one launch"""
    _chk(dout)
    _chk_ids(ids)
    E = dout.shape[-1]
    dW = torch.empty((V, E), dtype=torch.float32, device=dout.device)
    _l.check(_lib().vqf_embed_dropout_bwd(_ptr(dout), ctypes.c_void_p(ids.data_ptr()), ids.numel(), V, E, _keep_ptr(keep), int(seed),
                                          float(p_drop), _ptr(dW), _stream()), "vqf_embed_dropout_bwd")
    return dW


def embed_tanh_bwd(dout, out, ids, V, time_major=False, lens=None):
    """-> dW (V,E): deterministic segment sum of dout * (1 - out^2) over the tokens of each id (out=None: of dout, the plain lookup);
    time_major: dout / out are (Tq, N, E) for ids (N, Tq); lens (N) int32: the tokens at positions >= lens[n] add to no row"""
    _chk(dout, out)
    _chk_ids(ids)
    E = dout.shape[-1]
    dW = torch.empty((V, E), dtype=torch.float32, device=dout.device)
    if lens is not None:
        if out is None or time_major or ids.dim() != 2:
            raise _l.VqfError("embed_tanh_bwd: lens goes with (N, Tq) ids, tanh and sample-major rows")
        N, Tq = ids.shape
        _chk_lens(lens, N, "embed_tanh_bwd")
        _l.check(_lib().vqf_embed_tanh_bwd_len(_ptr(dout), _ptr(out), ctypes.c_void_p(ids.data_ptr()), _ptr(lens), N, Tq, V, E,
                                               _ptr(dW), _stream()), "vqf_embed_tanh_bwd_len")
        return dW
    if time_major:
        N, Tq = ids.shape
        _l.check(_lib().vqf_embed_tanh_bwd_tm(_ptr(dout), _ptr(out), ctypes.c_void_p(ids.data_ptr()), N, Tq, V, E, _ptr(dW),
                                              _stream()), "vqf_embed_tanh_bwd_tm")
        return dW
    if out is None:
        _l.check(_lib().vqf_embed_bwd(_ptr(dout), ctypes.c_void_p(ids.data_ptr()), ids.numel(), V, E, _ptr(dW), _stream()),
                 "vqf_embed_bwd")
    else:
        _l.check(_lib().vqf_embed_tanh_bwd(_ptr(dout), _ptr(out), ctypes.c_void_p(ids.data_ptr()), ids.numel(), V, E, _ptr(dW),
                                           _stream()), "vqf_embed_tanh_bwd")
    return dW


# ---------------------------------------------------------------------------
# input staging (data_loader.py:30-32)
def feat_transpose(src, out=None, bf16=False):
    """src (N, D, L) fp32 as stored by the feature extractor -> (N, L, D) fp32 | bf16."""
    _chk(src)
    if src.dim() != 3:
        raise _l.VqfError("feat_transpose: (N, D, L) expected")
    N, D, L = src.shape
    dt = torch.bfloat16 if bf16 else torch.float32
    if out is None:
        out = torch.empty((N, L, D), dtype=dt, device=src.device)
    elif out.shape != (N, L, D) or out.dtype != dt or not out.is_contiguous() or not out.is_cuda:
        raise _l.VqfError("feat_transpose: out must be a contiguous (N, L, D) %s GPU tensor" % dt)
    _l.check(_lib().vqf_feat_transpose(_ptr(src), N, D, L, 1 if bf16 else 0, _ptr(out), _stream()),
             "vqf_feat_transpose")
    return out


def region_rows_stage_supported(U, R, L, D):
    """The shapes vqf_region_rows_stage takes (include/vqa_fusion.h); no GPU needed."""
    return 1 <= int(U) <= 65535 and 1 <= int(R) < (1 << 29) and 1 <= int(L) <= 1024 and int(D) % 4 == 0 and 4 <= int(D) <= 65536


def region_rows_stage(src, roff=None, L=None, out=None):
    """src (R, D) fp32 | fp16, the real rows of every image one after the other, as the H2D copy left them.
    roff None -> (R, D) fp32, the same rows widened (a copy for fp32).  roff (U + 1,) int32 with L -> (U, L, D) fp32: image u's rows
    l < its count are src[start + l], the others exact +0.0 rows (nothing read there); roff is clamped in the kernel."""
    if not torch.is_tensor(src) or not src.is_cuda:
        raise _l.VqfError("vqa fusion ops need GPU tensors (HIP extension is the only path; no CPU fallback)")
    if src.dtype not in (torch.float32, torch.float16) or src.dim() != 2 or not src.is_contiguous():
        raise _l.VqfError("region_rows_stage: src must be a contiguous (R, D) fp32 or fp16 tensor")
    R, D = src.shape
    if roff is None:
        U, Lk, shape = 1, 1, (R, D)
    else:
        if L is None or isinstance(L, bool) or not isinstance(L, int):
            raise _l.VqfError("region_rows_stage: the padded form needs L (a Python int)")
        if not torch.is_tensor(roff) or roff.device != src.device or roff.dtype != torch.int32 or not roff.is_contiguous() or \
                roff.dim() != 1:
            raise _l.VqfError("region_rows_stage: roff must be a contiguous (U + 1,) int32 tensor on src's device")
        U, Lk = roff.numel() - 1, L
        shape = (U, Lk, D)
    if not region_rows_stage_supported(U, R, Lk, D):
        raise _l.VqfError("region_rows_stage: 1 <= U <= 65535 images, 1 <= R < 2^29 rows, 1 <= L <= 1024 and D %% 4 == 0, "
                          "4 <= D <= 65536 are supported (got U=%d, R=%d, L=%d, D=%d)" % (U, R, Lk, D))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=src.device)
    else:
        _chk(out)
        if out.device != src.device or out.numel() != math.prod(shape):
            raise _l.VqfError("region_rows_stage: out must be a contiguous fp32 tensor of %s on src's device (roff has %d entries)"
                              % (shape, 0 if roff is None else roff.numel()))
    _l.check(_lib().vqf_region_rows_stage(_ptr(src), 1 if src.dtype == torch.float16 else 0, _ptr(roff), U, R, Lk, D, _ptr(out),
                                          _stream()), "vqf_region_rows_stage")
    return out


# ---------------------------------------------------------------------------
# training-step tail (solver.py:25-29,91-94)
def _loss_ws(N, A, device):
    nbytes = int(_lib().vqf_loss_ws_bytes(N, A))
    return workspace(device, nbytes), nbytes


def ce_loss(logits, target, want_grad=True):
    """-> (loss (1,), dlogits | None): nn.CrossEntropyLoss() forward and gradient in one pass."""
    _chk(logits)
    if logits.dim() != 2 or target.shape != (logits.shape[0],):
        raise _l.VqfError("ce_loss: logits (N,A) and targets (N,) expected")
    if not target.is_cuda or target.dtype != torch.int64 or not target.is_contiguous():
        raise _l.VqfError("ce_loss: contiguous int64 GPU targets expected")
    N, A = logits.shape
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    d = torch.empty_like(logits) if want_grad else None
    ws, nb = _loss_ws(N, A, logits.device)
    _l.check(_lib().vqf_ce_loss(_ptr(logits), _ptr(target), N, A, _ptr(loss), _ptr(d), _ptr(ws), nb, _stream()),
             "vqf_ce_loss")
    return loss, d


def _chk_totals(name, dev, accumulate, **bufs):
    """the device totals of the evaluation tail: counts (2,) / rows (1,) int64, sums (1,) float64, acc / loss (1,) float32"""
    want = {"counts": (torch.int64, 2), "rows": (torch.int64, 1), "loss_sum": (torch.float64, 1), "score_sum": (torch.float64, 1),
            "acc": (torch.float32, 1), "loss": (torch.float32, 1), "loss_out": (torch.float32, 1)}
    for k, t in bufs.items():
        if t is None:
            continue
        dt, n = want[k]
        if not t.is_cuda or t.device != dev or t.dtype != dt or t.numel() != n or not t.is_contiguous():
            raise _l.VqfError("%s: %s must be a contiguous %s GPU tensor of %d element(s) on the inputs' device"
                              % (name, k, dt, n))
    return 1 if accumulate else 0


def ce_loss_pred(logits, target, want_grad=True, want_pred=True, counts=None, loss_sum=None, acc=None, accumulate=False,
                 loss_out=None):
    """-> (loss (1,), dlogits | None, pred (N,) int64 | None): ce_loss (the same bits) with the row arg-max riding in its
    row pass.  counts (2,) int64 = [rows with pred == target, rows with target != -100], loss_sum (1,) float64 = the sum of
    the row losses: written, or added to when `accumulate`; acc (1,) fp32 = this call's hits / counted rows."""
    _chk(logits)
    if logits.dim() != 2 or target.shape != (logits.shape[0],):
        raise _l.VqfError("ce_loss_pred: logits (N,A) and targets (N,) expected")
    if not target.is_cuda or target.dtype != torch.int64 or not target.is_contiguous():
        raise _l.VqfError("ce_loss_pred: contiguous int64 GPU targets expected")
    acc_flag = _chk_totals("ce_loss_pred", logits.device, accumulate, counts=counts, loss_sum=loss_sum, acc=acc,
                           loss_out=loss_out)
    N, A = logits.shape
    loss = loss_out if loss_out is not None else torch.empty(1, dtype=torch.float32, device=logits.device)
    d = torch.empty_like(logits) if want_grad else None
    pred = torch.empty(N, dtype=torch.int64, device=logits.device) if want_pred else None
    nb = 8 * N
    ws = workspace(logits.device, nb)
    _l.check(_lib().vqf_ce_loss_pred(_ptr(logits), _ptr(target), N, A, _ptr(loss), _ptr(d), _ptr(pred), _ptr(counts),
                                     _ptr(loss_sum), _ptr(acc), acc_flag, _ptr(ws), nb, _stream()), "vqf_ce_loss_pred")
    return loss, d, pred


def answer_match_rows(logp, target, want_score=True, counts=None, score_sum=None, loss=None, loss_sum=None, acc=None,
                      accumulate=False):
    """-> (pred (N,), tpred (N,) int64, score (N,) fp32 | None) for the soft-target models: the arg-max of the log-probs, the
    arg-max of the soft target (solver.py:100) and score = target[n, pred[n]].  counts = [rows with pred == tpred, N],
    score_sum = the sum of score, loss_sum = N * loss[0] (`loss`: the device scalar kldiv_loss returned): written, or
    added to when `accumulate`; acc (1,) fp32 = this call's hits / N."""
    _chk(logp, target)
    if logp.dim() != 2 or target.shape != logp.shape:
        raise _l.VqfError("answer_match_rows: log-probs and targets of the same (N,A) shape expected")
    acc_flag = _chk_totals("answer_match_rows", logp.device, accumulate, counts=counts, score_sum=score_sum, loss=loss,
                           loss_sum=loss_sum, acc=acc)
    N, A = logp.shape
    pred = torch.empty(N, dtype=torch.int64, device=logp.device)
    tpred = torch.empty(N, dtype=torch.int64, device=logp.device)
    score = torch.empty(N, dtype=torch.float32, device=logp.device) if want_score else None
    nb = 8 * N
    ws = workspace(logp.device, nb)
    _l.check(_lib().vqf_answer_match_rows(_ptr(logp), _ptr(target), N, A, _ptr(pred), _ptr(tpred), _ptr(score),
                                          _ptr(counts), _ptr(score_sum), _ptr(loss), _ptr(loss_sum), _ptr(acc), acc_flag,
                                          _ptr(ws), nb, _stream()), "vqf_answer_match_rows")
    return pred, tpred, score


def bce_logits_loss(logits, target, scale, want_grad=True, want_pred=True, rows=None, score_sum=None, loss_sum=None, acc=None,
                    accumulate=False, loss_out=None):
    """-> (loss (1,), dlogits | None, pred (N,) int64 | None, score (N,) fp32 | None): binary cross-entropy with logits on soft
    answers, loss = scale * the sum over all elements of max(x,0) - x t + log1p(exp(-|x|)), dlogits = (sigmoid(x) - t) * scale,
    with the row arg-max and score = t[n, pred[n]] from the same row pass.  target: (N, A) fp32, or a SoftAnswers (by
    definition the call on target.dense(A); the dense tensor is never formed).  rows (1,) int64 = N, score_sum (1,) float64 =
    the sum of score, loss_sum (1,) float64 = N * loss: written, or added to when `accumulate`; acc (1,) fp32 = this call's
    mean score."""
    _chk(logits)
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise _l.VqfError("bce_logits_loss: non-empty logits (N,A) expected")
    N, A = logits.shape
    sparse = isinstance(target, SoftAnswers)
    if sparse:
        check_soft_answers("bce_logits_loss", target, N, logits.device)
        ids, scores = target.ids.contiguous(), target.scores.contiguous()
    else:
        if not torch.is_tensor(target):
            raise _l.VqfError("bce_logits_loss: target must be a (N,A) fp32 tensor or a SoftAnswers, got %s"
                              % type(target).__name__)
        _chk(target)
        if target.shape != logits.shape or target.device != logits.device:
            raise _l.VqfError("bce_logits_loss: logits and targets of the same (N,A) shape on one device expected")
    acc_flag = _chk_totals("bce_logits_loss", logits.device, accumulate, rows=rows, score_sum=score_sum, loss_sum=loss_sum,
                           acc=acc, loss_out=loss_out)
    loss = loss_out if loss_out is not None else torch.empty(1, dtype=torch.float32, device=logits.device)
    d = torch.empty_like(logits) if want_grad else None
    pred = torch.empty(N, dtype=torch.int64, device=logits.device) if want_pred else None
    score = torch.empty(N, dtype=torch.float32, device=logits.device) if want_pred else None
    nb = int(_lib().vqf_bce_loss_ws_bytes(N))
    ws = workspace(logits.device, nb)
    tail = (float(scale), _ptr(loss), _ptr(d), _ptr(pred), _ptr(score), _ptr(rows), _ptr(score_sum), _ptr(loss_sum), _ptr(acc),
            acc_flag, _ptr(ws), nb, _stream())
    if sparse:
        _l.check(_lib().vqf_bce_loss_sparse(_ptr(logits), _ptr(ids), 1 if ids.dtype == torch.int64 else 0, _ptr(scores),
                                            ids.shape[1], N, A, *tail), "vqf_bce_loss_sparse")
    else:
        _l.check(_lib().vqf_bce_loss(_ptr(logits), _ptr(target), N, A, *tail), "vqf_bce_loss")
    return loss, d, pred, score


def topk_rows_supported(W, k):
    return bool(_lib().vqf_topk_rows_supported(int(W), int(k)))


def topk_rows(x, k, mode=0):
    """x (R, W) fp32, unit stride along W (rows may be strided: a column slice of a wider matrix) -> (idx (R, k) int64,
    val (R, k) fp32), every row's k largest entries in descending order, ties to the lowest index, NaN first.
    mode 0: the entries; mode 1: their softmax probabilities over the whole row."""
    if not x.is_cuda:
        raise _l.VqfError("vqa fusion ops need GPU tensors (HIP extension is the only path; no CPU fallback)")
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise _l.VqfError("topk_rows: a non-empty fp32 (R, W) tensor expected")
    R, W = x.shape
    ldx = x.stride(0) if R > 1 else W
    if x.stride(1) != 1 or ldx < W:
        raise _l.VqfError("topk_rows: unit stride along the row and a row pitch >= W expected")
    k = int(k)
    idx = torch.empty(R, max(k, 0), dtype=torch.int64, device=x.device)
    val = torch.empty(R, max(k, 0), dtype=torch.float32, device=x.device)
    _l.check(_lib().vqf_topk_rows(_ptr(x), R, W, ldx, k, int(mode), _ptr(idx), _ptr(val), _stream()), "vqf_topk_rows")
    return idx, val


def kldiv_loss(logp, target, want_grad=True, loss_out=None):
    """-> (loss (1,), dlogp | None): nn.KLDivLoss() (element-wise mean) forward and gradient.
    loss_out: a (1,) fp32 GPU tensor to write the loss into (the evaluator's device record) instead of a new one."""
    _chk(logp, target)
    if logp.dim() != 2 or target.shape != logp.shape:
        raise _l.VqfError("kldiv_loss: log-probs and targets of the same (N,A) shape expected")
    _chk_totals("kldiv_loss", logp.device, False, loss_out=loss_out)
    N, A = logp.shape
    loss = loss_out if loss_out is not None else torch.empty(1, dtype=torch.float32, device=logp.device)
    d = torch.empty_like(logp) if want_grad else None
    ws, nb = _loss_ws(N, A, logp.device)
    _l.check(_lib().vqf_kldiv_loss(_ptr(logp), _ptr(target), N, A, _ptr(loss), _ptr(d), _ptr(ws), nb, _stream()),
             "vqf_kldiv_loss")
    return loss, d


def _optim_table(what, params, grads, exp_avgs, second):
    n = len(params)
    if not (len(grads) == len(exp_avgs) == len(second) == n):
        raise _l.VqfError("%s: list lengths differ" % what)
    tab = (_l.AdamTensor * max(n, 1))()
    for i, (p, g, m, v) in enumerate(zip(params, grads, exp_avgs, second)):
        _chk(p, g, m, v)
        if not (p.numel() == g.numel() == m.numel() == v.numel()):
            raise _l.VqfError("%s: tensor %d: sizes differ" % (what, i))
        tab[i].param, tab[i].grad = p.data_ptr(), g.data_ptr()
        tab[i].exp_avg, tab[i].exp_avg_sq, tab[i].n = m.data_ptr(), v.data_ptr(), p.numel()
    return tab, n


def _chk_device_scalar(what, t, device):
    """a one-element fp32 tensor on `device`: what the kernels read a scale / clip coefficient from"""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.numel() == 1 and t.device == device):
        raise _l.VqfError("%s: a one-element fp32 tensor on %s expected" % (what, device))


def adam_step(params, grads, exp_avgs, exp_avg_sqs, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
              grad_scale=None):
    """In-place torch.optim.Adam update of every tensor in the lists (one launch per 32 tensors).  grad_scale: a one-element
    fp32 GPU tensor (the coefficient of grad_norm_clip); the update then sees g * grad_scale, the gradients stay as they are."""
    tab, n = _optim_table("adam_step", params, grads, exp_avgs, exp_avg_sqs)
    if n == 0:
        return
    args = (ctypes.cast(tab, ctypes.c_void_p), n, float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
            int(step))
    if grad_scale is None:
        _l.check(_lib().vqf_adam_step(*args, _stream()), "vqf_adam_step")
    else:
        _chk_device_scalar("adam_step: grad_scale", grad_scale, params[0].device)
        _l.check(_lib().vqf_adam_step_scaled(*args, _ptr(grad_scale), _stream()), "vqf_adam_step_scaled")


def adamax_step(params, grads, exp_avgs, exp_infs, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
                grad_scale=None):
    """In-place torch.optim.Adamax update of every tensor in the lists (one launch per 32 tensors); grad_scale as in adam_step."""
    tab, n = _optim_table("adamax_step", params, grads, exp_avgs, exp_infs)
    if n == 0:
        return
    if grad_scale is not None:
        _chk_device_scalar("adamax_step: grad_scale", grad_scale, params[0].device)
    _l.check(_lib().vqf_adamax_step(ctypes.cast(tab, ctypes.c_void_p), n, float(lr), float(beta1), float(beta2), float(eps),
                                    float(weight_decay), int(step), _ptr(grad_scale), _stream()), "vqf_adamax_step")


def _grad_table(what, grads):
    """-> (VqfAdamTensor array with grad and n filled in, count, device): fp32 contiguous GPU tensors on one device"""
    n = len(grads)
    tab = (_l.AdamTensor * max(n, 1))()
    for i, g in enumerate(grads):
        _chk(g)
        if g.device != grads[0].device:
            raise _l.VqfError("%s: gradients on one device expected" % what)
        tab[i].grad, tab[i].n = g.data_ptr(), g.numel()
    return tab, n, (grads[0].device if n else None)


def grad_norm_clip(grads, max_norm):
    """-> (norm, coef), 0-d fp32 GPU tensors: the 2-norm over every tensor of `grads` and min(1, max_norm / (norm + 1e-6)) as
    torch.nn.utils.clip_grad_norm_ forms it in fp32.  Nothing is scaled and nothing is read back; two calls on the same
    memory give the same bits."""
    max_norm = float(max_norm)
    if not max_norm > 0.0:
        raise ValueError("grad_norm_clip: max_norm must be > 0, got %r" % (max_norm,))
    tab, n, device = _grad_table("grad_norm_clip", grads)
    if n == 0:
        raise _l.VqfError("grad_norm_clip: no gradients")
    out = torch.empty(2, dtype=torch.float32, device=device)
    nb = int(_lib().vqf_grad_norm_ws_bytes(ctypes.cast(tab, ctypes.c_void_p), n))
    ws = workspace(device, nb)
    _l.check(_lib().vqf_grad_norm_clip(ctypes.cast(tab, ctypes.c_void_p), n, max_norm, _ptr(out), out.data_ptr() + 4, _ptr(ws),
                                       nb, _stream()), "vqf_grad_norm_clip")
    return out[0], out[1]


def grad_scale_(grads, scale):
    """g *= scale for every tensor of `grads`, in place; scale: a one-element fp32 GPU tensor (one fp32 multiply per element)."""
    tab, n, device = _grad_table("grad_scale_", grads)
    if n == 0:
        return
    _chk_device_scalar("grad_scale_: scale", scale, device)
    _l.check(_lib().vqf_grad_scale(ctypes.cast(tab, ctypes.c_void_p), n, _ptr(scale), _stream()), "vqf_grad_scale")


# ---------------------------------------------------------------------------
# HBM yardsticks (measurement only: bench.py's hbm_yardsticks)
def hbm_copy(src, dst, nt=False):
    """dst = src with the library's plain 16-B-per-lane grid-stride copy kernel (any dtype, same byte count)."""
    nbytes = src.numel() * src.element_size()
    if not (src.is_cuda and dst.is_cuda and src.is_contiguous() and dst.is_contiguous()) or dst.numel() * dst.element_size() != nbytes:
        raise _l.VqfError("hbm_copy: contiguous GPU tensors of the same byte count expected")
    _l.check(_lib().vqf_hbm_copy(_ptr(src), _ptr(dst), nbytes, int(bool(nt)), _stream()), "vqf_hbm_copy")
    return dst


def hbm_read_sweep(src, nt=False, out=None):
    """-> per-workgroup sums (fp32) of a pure read stream over `src` (fp32, contiguous)."""
    _chk(src)
    nbytes = src.numel() * 4
    nb = int(_lib().vqf_hbm_read_sweep_blocks(nbytes))
    if out is None:
        out = torch.empty(nb, dtype=torch.float32, device=src.device)
    _l.check(_lib().vqf_hbm_read_sweep(_ptr(src), nbytes, int(bool(nt)), _ptr(out), _stream()), "vqf_hbm_read_sweep")
    return out


# ---------------------------------------------------------------------------
def prof_enable(on=True, min_mnk=0):
    """hipEvent brackets around the library's launches.  min_mnk > 0: only GEMM launches with M * N * K >= min_mnk (an
    event pair costs the stream ~6-10 us between two kernels, so a timed region brackets its dominant launches only)."""
    _lib().vqf_prof_filter(int(min_mnk))
    _lib().vqf_prof_enable(int(on))


def prof_reset():
    _lib().vqf_prof_reset()


def prof_report():
    """{kernel name: (launches, total_ms)} for kernels launched since the last reset."""
    lib = _lib()
    out = {}
    for i in range(lib.vqf_prof_num_kernels()):
        n = ctypes.c_longlong(0)
        ms = ctypes.c_double(0.0)
        _l.check(lib.vqf_prof_get(i, ctypes.byref(n), ctypes.byref(ms)), "vqf_prof_get")
        if n.value:
            out[lib.vqf_prof_kernel_name(i).decode()] = (n.value, ms.value)
    return out


def prof_shape(kernel, d0=-1, d1=-1, d2=-1):
    """(launches, total_ms) of the launches of `kernel` (profiler name as in prof_report(), or id) whose shape tag
    matches (GEMMs tag M, N, K; -1 = any) since the last reset."""
    lib = _lib()
    if isinstance(kernel, str):
        names = [lib.vqf_prof_kernel_name(i).decode() for i in range(lib.vqf_prof_num_kernels())]
        if kernel not in names:
            raise _l.VqfError("prof_shape: no kernel named %r" % kernel)
        kernel = names.index(kernel)
    n = ctypes.c_longlong(0)
    ms = ctypes.c_double(0.0)
    _l.check(lib.vqf_prof_get_shape(int(kernel), int(d0), int(d1), int(d2), ctypes.byref(n), ctypes.byref(ms)),
             "vqf_prof_get_shape")
    return n.value, ms.value


def prof_gemm(ta, tb, M, N, K):
    """(launches, total_ms) of the GEMM launches with this layout and shape since the last reset."""
    lib = _lib()
    n = ctypes.c_longlong(0)
    ms = ctypes.c_double(0.0)
    _l.check(lib.vqf_prof_get_shape(2 * int(bool(ta)) + int(bool(tb)), M, N, K, ctypes.byref(n),
                                    ctypes.byref(ms)), "vqf_prof_get_shape")
    return n.value, ms.value
