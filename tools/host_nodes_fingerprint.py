#!/usr/bin/env python3
"""Fingerprint of the host glue (host/functions.py and the models' forward bodies): for a list of small cases that take every
branch of that glue, the ordered log of the ops.* calls the host modules make during two train steps and the sha256 of every
output and parameter gradient after each step.  Two commits whose Python differs only in how the glue is written must print the
same file, byte for byte.

    python tools/host_nodes_fingerprint.py --out fp.txt [--log calls.txt] [--only SUBSTR]

--out: per case the number of calls, the sha256 of the call log, the calls per function and the tensor hashes (small: the file
that is kept under profiles/).  --log: the call logs themselves and the hash of every single gradient (what to diff when two --out files differ).  Each log line is
`function | stream | arguments | result`: tensors as shape:dtype:strides, scalars and flags by value (bound to the callee's signature, defaults filled in), the stream as `main` (the
caller's) or `side`.  The tool imports only the package's public names; it runs in one process and stops at the first error.
After the cases it asserts from the logs that each branch the cases are there for was taken."""
import argparse
import collections
import hashlib
import inspect
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vqa_amd as vqa                                                                   # noqa: E402
from vqa_amd import functions as F, ops                                                  # noqa: E402

DEV = "cuda:0"
LOG = []            # the current case's call log
MAIN = [None]       # the caller's stream


def _desc(v):
    if torch.is_tensor(v):
        return "%s:%s:%s" % (tuple(v.shape), str(v.dtype)[6:], tuple(v.stride()))
    if v is None or isinstance(v, (bool, int, float, str)):
        return repr(v)
    if isinstance(v, (list, tuple)):
        return "[" + ",".join(_desc(x) for x in v) + "]"
    if isinstance(v, dict):
        return "{" + ",".join("%s=%s" % (k, _desc(x)) for k, x in sorted(v.items())) + "}"
    return "<%s>" % type(v).__name__


def _logged(name, real):
    try:
        sig = inspect.signature(real)
    except (TypeError, ValueError):
        sig = None

    def call(*a, **kw):
        # the arguments as the callee receives them, defaults filled in, described before the call (a list may be an output)
        if sig is not None:
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            args = ",".join("%s=%s" % (k, _desc(v)) for k, v in bound.arguments.items())
        else:
            args = ",".join([_desc(x) for x in a] + ["%s=%s" % (k, _desc(x)) for k, x in sorted(kw.items())])
        stream = "main" if torch.cuda.current_stream() == MAIN[0] else "side"
        out = real(*a, **kw)
        LOG.append("%s | %s | %s | %s" % (name, stream, args, _desc(out)))
        return out
    return call


class _OpsProxy:
    """`ops` as a host module sees it: every public callable logs its call; everything else is the module's own attribute"""

    def __init__(self):
        self._wrapped = {}

    def __getattr__(self, name):
        real = getattr(ops, name)
        if name.startswith("_") or not callable(real):
            return real
        if name not in self._wrapped:
            self._wrapped[name] = _logged(name, real)
        return self._wrapped[name]


def _install_proxy():
    import importlib
    pkg = vqa.__name__
    for name in ("mfb", "mhb_coAtt", "hieCoAtten", "hie_ladder", "networks", "modules", "functions"):
        importlib.import_module("%s.host.%s" % (pkg, name))
    proxy, n = _OpsProxy(), 0
    for name, mod in list(sys.modules.items()):
        if name.startswith(pkg + ".host.") and mod is not ops and getattr(mod, "ops", None) is ops:
            mod.ops = proxy
            n += 1
    assert n >= 4, "the host modules' `ops` was not found"


def _sha(t):
    if t is None:
        return "none"
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------------------------ inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _counts(U, L):
    return torch.tensor(([L - 1, 1, L, 7] + torch.randint(1, L + 1, (max(U - 4, 0),), generator=_gen(11)).tolist())[:U], dtype=torch.int64)


def _pack(img, counts):
    rows = torch.cat([img[u, :int(c)] for u, c in enumerate(counts)], 0)
    off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)])
    return vqa.PackedRegions(rows.to(DEV), off.to(DEV), img.shape[1])


INDEX7 = [0, 2, 0, 2, 2, 0, 0]          # U = 3, N = 7, image 1 without a question


def _regions(form, N, L, D):
    """-> (img_features in the call form, img_index or None, U)"""
    U = 3 if form in ("index", "packed-index") else N
    img = torch.rand(U, L, D, generator=_gen(3))
    idx = torch.tensor(INDEX7, device=DEV) if U != N else None
    counts = _counts(U, L)
    if form in ("plain", "index"):
        return img.to(DEV), idx, U
    if form == "pair":
        return (img.to(DEV), counts.to(DEV)), idx, U
    return _pack(img, counts), idx, U


def _mask(g, *shape, p=0.1):
    return (torch.rand(shape, generator=g) >= p).to(torch.uint8).to(DEV)


# ------------------------------------------------------------------------------------------------------------------ cases
def _cfg(model_name, hidden, glove=False):
    return types.SimpleNamespace(q_vocab_size=50, a_vocab_size=30, emb_dim=20, hidden_dim=hidden, num_layers=1, model_name=model_name,
                                 glove=glove, img_feature_channel=96, img_feature_dim=20)


def mfb_case(name, N=8, model_name="mfb-baseline", hidden=64, form="plain", mode="philox", attrs=None, switches=(), cls="MFB",
             glove=False, bf16_features=False):
    """MFB / MHBCoAtt: L = 20, D = 96, T = 14.  attrs: model attributes; switches: (owner, attribute, value) class switches"""
    def run():
        L, D, T = 20, 96, 14
        if form in ("index", "packed-index"):
            assert N == 7
        model = getattr(vqa, cls)(_cfg(model_name, hidden, glove)).to(DEV)
        for k, v in (attrs or {}).items():
            assert hasattr(model, k), k
            setattr(model, k, v)
        model.train(mode != "eval")
        feats, idx, U = _regions(form, N, L, D)
        if bf16_features:                                          # bf16 feature storage: the projection takes the batch as it is
            feats = feats.to(torch.bfloat16)
        q = torch.randint(1, 50, (N, T), generator=_gen(4)).to(DEV)
        if mode == "masks":
            g = _gen(5)
            masks = {"m1": _mask(g, N * L, 5000), "m2": _mask(g, N, 5000), "m3": _mask(g, N, 5000), "l": _mask(g, N * T, hidden, p=0.3)}
            model.set_keep_masks(**masks)
        kw = {} if idx is None else {"img_index": idx}
        if glove:
            kw["glove_matrix"] = torch.rand(N, T, 20, generator=_gen(6)).to(DEV)
        return model, lambda: model(feats, q, **kw)
    return name, run, switches


def mhb_case(name):
    def run():
        N, L, D, T = 8, 20, 96, 14
        model = vqa.MHB(_cfg("mhb", 64)).to(DEV).train()
        img = torch.rand(N, L, D, generator=_gen(3)).to(DEV)
        q = torch.randint(1, 50, (N, T), generator=_gen(4)).to(DEV)
        qlen = torch.tensor([T, 1, 3, 14, 7, 2, 9, 5], device=DEV)
        return model, lambda: model(img, q, qlen)
    return name, run, ()


def hie_case(name, kind, fused=True):
    def run():
        N, L, T, D, E = 8, 20, 6, 48, 64
        img = torch.rand(N, L, D, generator=_gen(3)).to(DEV)
        q = torch.randint(1, 50, (N, T), generator=_gen(4)).to(DEV)
        if kind == "hie":
            model = vqa.HieCoAtten(block_num=L, word_num=T, img_size=D, vocab_size=50, embed_size=E, output_size=30).to(DEV).train()
            model.fused = fused
        elif kind == "attnet":
            model = vqa.AttentionNet(block_num=L, word_num=T, img_size=D, vocab_size=50, embed_size=E, att_num=2, output_size=30).to(DEV).train()
        else:
            model = vqa.iBOWIMG(D, 50, E, 30).to(DEV).train()
            img = img[:, 0].contiguous()
        return model, lambda: model(img, q)
    return name, run, ()


def ladder_case(name, coatt="parallel", form="plain", mode="philox", lens=True, packed_coatt=False, N=8):
    def run():
        L, T, D, E, H = 20, 6, 48, 64, 48
        kw = {"packed_coatt": True} if packed_coatt else {}
        model = vqa.HieCoAttenLadder(block_num=L, img_size=D, vocab_size=50, embed_size=E, hidden_size=H, output_size=30, coatt=coatt,
                                     **kw).to(DEV)
        model.train(mode in ("philox", "masks"))
        feats, idx, U = _regions(form, N, L, D)
        q = torch.randint(1, 50, (N, T), generator=_gen(4)).to(DEV)
        qlen = torch.tensor(([2, 1, T] + torch.randint(1, T + 1, (N,), generator=_gen(7)).tolist())[:N], device=DEV) if lens else None
        if mode in ("masks", "eval-masks"):
            g = _gen(5)
            model.set_keep_masks(img=_mask(g, U * L, E, p=0.5), word=_mask(g, N * T, E, p=0.5), ans_w=_mask(g, N, E, p=0.5),
                                 ans_p=_mask(g, N, 2 * E, p=0.5), ans_s=_mask(g, N, 2 * E, p=0.5), ans_h=_mask(g, N, H, p=0.5))
        return model, lambda: model(feats, q, qlen, idx)
    return name, run, ()


def _cases():
    SS, LB = sys.modules[vqa.MFB.__module__]._SideStream, F.LstmBatchFn
    c = [
        mfb_case("mfb/fp32/N8"),
        mfb_case("mfb/fp32/N6", N=6),
        mfb_case("mfb/fp32/N8/multilayer", model_name="mfb-multilayer"),
        mfb_case("mfb/fp32/N8/masks", mode="masks"),
        mfb_case("mfb/fp32/N8/eval", mode="eval"),
        mfb_case("mfb/fp32/N8/same-stream", attrs={"overlap_streams": "same-stream"}),
        mfb_case("mfb/fp32/N8/same-stream/nodefer", attrs={"overlap_streams": "same-stream"}, switches=((SS, "DEFER", False),)),
        mfb_case("mfb/fp32/N8/one-node", attrs={"overlap_streams": False}),
        mfb_case("mfb/fp32/N8/nofold", attrs={"fold_norm": False}),
        mfb_case("mfb/fp32/N8/pruned", attrs={"pruned": True}),
        mfb_case("mfb/fp32/N8/pruned/masks", attrs={"pruned": True}, mode="masks"),
        mfb_case("mfb/fp32/N8/cu128", attrs={"side_cu_limit": 128}),
        mfb_case("mfb/fp32/N8/final-two-streams", switches=((F.FinalMfbFn, "TWO_STREAMS", True),)),
        mfb_case("mfb/bf16/N8", attrs={"gemm_dtype": "bf16"}),
        mfb_case("mfb/bf16/N8/masks", attrs={"gemm_dtype": "bf16"}, mode="masks"),
        mfb_case("mfb/bf16/N8/multilayer", model_name="mfb-multilayer", attrs={"gemm_dtype": "bf16"}),
        mfb_case("mfb/bf16/N8/nofuse-dp", attrs={"gemm_dtype": "bf16", "fuse_bf16_dp": False}),
        mfb_case("mfb/bf16/N8/nofuse-dp/same-stream", attrs={"gemm_dtype": "bf16", "fuse_bf16_dp": False, "overlap_streams": "same-stream"}),
        mfb_case("mfb/bf16/N8/side-bf16", attrs={"gemm_dtype": "bf16", "side_bf16": True}),
        mfb_case("mfb/bf16/N8/nofold", attrs={"gemm_dtype": "bf16", "fold_norm": False}),
        mfb_case("mfb/bf16/N8/bf16-features", attrs={"gemm_dtype": "bf16"}, bf16_features=True),
        mfb_case("mfb/bf16/N8/side-bf16/bf16-features", attrs={"gemm_dtype": "bf16", "side_bf16": True}, bf16_features=True),
        mfb_case("mfb/bf16/N8/nofuse-dp/same-stream/bf16-features", bf16_features=True,
                 attrs={"gemm_dtype": "bf16", "fuse_bf16_dp": False, "overlap_streams": "same-stream"}),
        mfb_case("mfb/bf16/N8/p-fp32", attrs={"gemm_dtype": "bf16"}, switches=((F.ImgFuseFn, "BF16_P", False),)),
        mfb_case("mfb/bf16-img/N8", attrs={"gemm_dtype": "bf16-img"}),
        mfb_case("mfb/bf16-att/N8", attrs={"gemm_dtype": "bf16-att"}),
        mfb_case("mfb/bf16-all/N8", attrs={"gemm_dtype": "bf16-all"}),
        mfb_case("mfb/bf16-all/N6", N=6, attrs={"gemm_dtype": "bf16-all"}),
        mfb_case("mfb/bf16-all/N8/multilayer", model_name="mfb-multilayer", attrs={"gemm_dtype": "bf16-all"}),
        mfb_case("mfb/bf16-all/N8/eval", attrs={"gemm_dtype": "bf16-all"}, mode="eval"),
        mfb_case("mfb/fp32/N128/H256/fused-step", N=128, hidden=256, switches=((LB, "FUSED_STEP", True),)),
        mfb_case("mfb/fp32/N128/H256/two-launch-step", N=128, hidden=256, switches=((LB, "FUSED_STEP", False),)),
        mfb_case("mfb/bf16/N128/H256", N=128, hidden=256, attrs={"gemm_dtype": "bf16"}),
        mfb_case("mfb/bf16/N128/H256/side-bf16", N=128, hidden=256, attrs={"gemm_dtype": "bf16", "side_bf16": True}),
        mfb_case("mfb/fp32/index", N=7, form="index"),
        mfb_case("mfb/fp32/index/one-node", N=7, form="index", attrs={"overlap_streams": False}),
        mfb_case("mfb/fp32/index/pruned", N=7, form="index", attrs={"pruned": True}),
        mfb_case("mfb/fp32/pair", form="pair"),
        mfb_case("mfb/fp32/pair/one-node/nofold", form="pair", attrs={"overlap_streams": False, "fold_norm": False}),
        mfb_case("mfb/fp32/packed", form="packed"),
        mfb_case("mfb/fp32/packed/same-stream", form="packed", attrs={"overlap_streams": "same-stream"}),
        mfb_case("mfb/fp32/packed-index", N=7, form="packed-index"),
        mfb_case("mfb/fp32/packed-coatt", form="packed", attrs={"packed_coatt": True}),
        mfb_case("mfb/fp32/packed-coatt/multilayer", model_name="mfb-multilayer", form="packed", attrs={"packed_coatt": True}),
    ]
    # regions_bf16: a bf16 P / dP on the region forms (N = 128: enough rows for the GEMM that stores P in bf16); regions_bf16_coatt:
    # the bf16 copy of R as well
    for tail, attrs in (("regions-bf16", {"regions_bf16": True}), ("regions-bf16-coatt", {"regions_bf16": True, "regions_bf16_coatt": True})):
        big = dict(N=128, hidden=256, form="packed")
        c += [mfb_case("mfb/fp32/N128/H256/pair/" + tail, N=128, hidden=256, form="pair", attrs=attrs),
              mfb_case("mfb/fp32/N128/H256/packed/" + tail, attrs=attrs, **big),
              mfb_case("mfb/fp32/N128/H256/packed-coatt/" + tail, attrs=dict(attrs, packed_coatt=True), **big)]
    co = dict(cls="MHBCoAtt", model_name="mhb_coAtt", hidden=256)
    c += [
        mfb_case("mhbcoatt/fp32", **co),
        mfb_case("mhbcoatt/fp32/masks", mode="masks", **co),
        mfb_case("mhbcoatt/fp32/eval", mode="eval", **co),
        mfb_case("mhbcoatt/fp32/one-node", attrs={"overlap_streams": False}, **co),
        mfb_case("mhbcoatt/bf16", attrs={"gemm_dtype": "bf16"}, **co),
        mfb_case("mhbcoatt/bf16/side-bf16", attrs={"gemm_dtype": "bf16", "side_bf16": True}, **co),
        mfb_case("mhbcoatt/bf16-all", attrs={"gemm_dtype": "bf16-all"}, **co),
        mfb_case("mhbcoatt/fp32/fix-orientation", attrs={"fix_lstm_orientation": True}, **co),
        mfb_case("mhbcoatt/bf16-all/fix-orientation", attrs={"gemm_dtype": "bf16-all", "fix_lstm_orientation": True}, **co),
        mfb_case("mhbcoatt/fp32/glove", glove=True, **co),
        mfb_case("mhbcoatt/fp32/packed", form="packed", **co),
        mfb_case("mhbcoatt/fp32/packed-coatt", form="packed", attrs={"packed_coatt": True}, **co),
        mhb_case("mhb/fp32"),
        hie_case("hiecoatten/fused", "hie", True),
        hie_case("hiecoatten/staged", "hie", False),
        hie_case("attentionnet", "attnet"),
        hie_case("ibowimg", "ibow"),
    ]
    for coatt in ("parallel", "alternating"):
        c += [
            ladder_case("ladder/%s/q_length" % coatt, coatt),
            ladder_case("ladder/%s/no_q_length" % coatt, coatt, lens=False),
            ladder_case("ladder/%s/masks" % coatt, coatt, mode="masks"),
            ladder_case("ladder/%s/eval" % coatt, coatt, mode="eval"),
            ladder_case("ladder/%s/eval/masks-ignored" % coatt, coatt, mode="eval-masks"),
            ladder_case("ladder/%s/index" % coatt, coatt, form="index", N=7),
            ladder_case("ladder/%s/pair" % coatt, coatt, form="pair"),
            ladder_case("ladder/%s/packed" % coatt, coatt, form="packed"),
            ladder_case("ladder/%s/packed/masks" % coatt, coatt, form="packed", mode="masks"),
        ]
    c += [ladder_case("ladder/alternating/packed-coatt", "alternating", form="packed", packed_coatt=True),
          ladder_case("ladder/alternating/packed-coatt/masks", "alternating", form="packed", packed_coatt=True, mode="masks")]
    return c


# ------------------------------------------------------------------------------------------------------------------ running
def _step(model, call, weights):
    model.zero_grad(set_to_none=True)
    outs = call()
    outs = [o for o in (outs if isinstance(outs, (tuple, list)) else (outs,)) if torch.is_tensor(o) and o.is_floating_point()]
    if not weights:                                                # fixed by seed and shape: the same numbers in both steps
        g = _gen(1234)
        weights.extend(torch.randn(o.shape, generator=g).to(DEV) for o in outs)
    loss = None
    for o, w in zip(outs, weights):
        if o.requires_grad:
            term = (o * w).sum()
            loss = term if loss is None else loss + term
    loss.backward()
    torch.cuda.synchronize()
    return outs


def run_case(name, build, switches):
    saved = [(o, a, getattr(o, a)) for o, a, _ in switches]
    try:
        for o, a, v in switches:
            setattr(o, a, v)
        torch.manual_seed(0)
        MAIN[0] = torch.cuda.current_stream()
        model, call = build()
        del LOG[:]
        lines, weights, detail = [], [], []
        for step in (1, 2):
            outs = _step(model, call, weights)
            for i, o in enumerate(outs):
                lines.append("step %d out %d %s %s" % (step, i, _desc(o), _sha(o)))
            grads = ["step %d grad %s %s" % (step, pn, _sha(p.grad)) for pn, p in model.named_parameters()]
            detail.extend(grads)
            lines.append("step %d grads %d sha256 %s" % (step, len(grads), hashlib.sha256("\n".join(grads).encode()).hexdigest()))
        return list(LOG), lines, detail
    finally:
        for o, a, v in saved:
            setattr(o, a, v)


def _names(log):
    return collections.Counter(l.split(" | ", 1)[0] for l in log)


def _check_branches(logs):
    """each branch the cases are there for, from the logs themselves"""
    def has(case, fn, text="", stream=None):
        return any(l.startswith(fn + " | ") and text in l and (stream is None or (" | %s | " % stream) in l) for l in logs[case])

    def differ(a, b):
        assert logs[a] != logs[b], "%s issues the calls of %s: its branch was not taken" % (a, b)

    if "mfb/fp32/N8" in logs:
        base = "mfb/fp32/N8"
        for other in ("N6", "N8/multilayer", "N8/masks", "N8/eval", "N8/same-stream", "N8/one-node", "N8/nofold", "N8/pruned", "N8/cu128",
                      "N8/final-two-streams", "index", "pair", "packed", "packed-coatt"):
            differ("mfb/fp32/" + other, base)
        differ("mfb/fp32/N8/same-stream/nodefer", "mfb/fp32/N8/same-stream")
        differ("mfb/fp32/N8/pruned/masks", "mfb/fp32/N8/pruned")
        differ("mfb/fp32/packed-index", "mfb/fp32/packed")
        differ("mfb/fp32/N128/H256/two-launch-step", "mfb/fp32/N128/H256/fused-step")
        assert has(base, "gemm", stream="side") and not has("mfb/fp32/N8/same-stream", "gemm", stream="side")
        assert not has("mfb/fp32/N8/one-node", "gemm", stream="side") and not _names(logs[base])["gemm_bf16"]
        assert has("mfb/fp32/N8/same-stream", "gemm", "out=(160, 5000)") and not has("mfb/fp32/N8/same-stream/nodefer", "gemm", "out=(160, 5000)")
        assert has("mfb/fp32/N8/cu128", "options", "gemm_cu_limit=128")
        assert has("mfb/fp32/N8/final-two-streams", "colsum", stream="side") and not has(base, "colsum", stream="side")
        assert has("mfb/fp32/N128/H256/fused-step", "lstm_step_fwd") and not has("mfb/fp32/N128/H256/two-launch-step", "lstm_step_fwd")
        assert has("mfb/fp32/index", "mfb_fuse_fwd_grouped") and has("mfb/fp32/pair", "mfb_fuse_fwd", "lens=(8,)")
        assert has("mfb/fp32/packed", "mfb_fuse_fwd_packed") and has("mfb/fp32/packed-coatt", "mfb_fuse_fwd_packed_rows")
        assert has("mfb/fp32/packed-index", "mfb_fuse_fwd_packed", "idx=(7,)")
        for form, fn in (("pair", "mfb_fuse_fwd"), ("packed", "mfb_fuse_fwd_packed"), ("packed-coatt", "mfb_fuse_fwd_packed_rows")):
            bf, co = ("mfb/fp32/N128/H256/%s/regions-bf16%s" % (form, t) for t in ("", "-coatt"))
            differ(co, bf)
            assert has(bf, fn, ", 5000):bfloat16:") and has(co, fn, ", 5000):bfloat16:") and not has("mfb/fp32/" + form, fn, ":bfloat16:")
            assert has(co, fn, "r_bf16=[]") and not has(bf, fn, "r_bf16=[]")
    if "mfb/bf16/N8" in logs:
        b = "mfb/bf16/N8"
        for other in ("N8/masks", "N8/multilayer", "N8/nofuse-dp", "N8/side-bf16", "N8/nofold", "N8/p-fp32", "N128/H256", "N8/bf16-features"):
            differ("mfb/bf16/" + other, b)
        for other in ("mfb/bf16-img/N8", "mfb/bf16-att/N8", "mfb/bf16-all/N8"):
            differ(other, b)
        differ("mfb/bf16/N8/nofuse-dp/same-stream", "mfb/bf16/N8/nofuse-dp")
        differ("mfb/bf16-all/N8/multilayer", "mfb/bf16-all/N8")
        differ("mfb/bf16/N8/side-bf16/bf16-features", "mfb/bf16/N8/side-bf16")
        differ("mfb/bf16/N8/nofuse-dp/same-stream/bf16-features", "mfb/bf16/N8/nofuse-dp/same-stream")
        assert has(b, "gemm_bf16", "out_bf16=True | None") and not has("mfb/bf16/N8/p-fp32", "gemm_bf16", "out_bf16=True")
        assert has("mfb/bf16/N128/H256", "gemm_bf16", "out_bf16=True | (2560, 5000):bfloat16")       # the bf16-stored projection itself
        assert has("mfb/bf16/N128/H256/side-bf16", "gemm_bf16", "out_bf16=True | (2560, 5000):bfloat16", stream="side")
        assert has("mfb/bf16/N8/side-bf16", "gemm_bf16", stream="side") and not has(b, "gemm_bf16", stream="side")
        assert has("mfb/bf16-img/N8", "gemm_bf16") and not has("mfb/bf16-img/N8", "gemm_bf16_rowscale")
        assert has("mfb/bf16-att/N8", "gemm_bf16_rowscale") and has(b, "gemm_bf16_rowscale")
        n8, n6 = _names(logs["mfb/bf16-all/N8"])["gemm_bf16"], _names(logs["mfb/bf16-all/N6"])["gemm_bf16"]
        assert 0 < n6 < n8, "N = 6 must take the fp32 fallback of LinearFn / FinalMfbFn (%d, %d bf16 products)" % (n6, n8)
        assert has("mfb/bf16-all/N8", "cast_bf16", "(112, 20):float32") and has("mfb/bf16-all/N8", "gemm_bf16", "(112, 24):bfloat16")
    if "mhbcoatt/fp32" in logs:
        b = "mhbcoatt/fp32"
        for other in ("fp32/masks", "fp32/eval", "fp32/one-node", "bf16", "bf16-all", "fp32/fix-orientation", "fp32/glove", "fp32/packed",
                      "fp32/packed-coatt"):
            differ("mhbcoatt/" + other, b)
        differ("mhbcoatt/bf16/side-bf16", "mhbcoatt/bf16")
        differ("mhbcoatt/bf16-all/fix-orientation", "mhbcoatt/bf16-all")
        assert has(b, "lstm_seq_fwd") and not has("mhbcoatt/fp32/fix-orientation", "lstm_seq_fwd")
        assert has("mhbcoatt/fp32/fix-orientation", "lstm_cell_fwd") and has("mhbcoatt/bf16-all", "lstm_seq_fwd", "bf16=True")
        assert has("mhb/fp32", "mfb_fuse_fwd", "want_zdrop=True") and has("mhb/fp32", "mfb_fuse_fwd", "cascade=(8, 5000)")
    if "hiecoatten/fused" in logs:
        differ("hiecoatten/staged", "hiecoatten/fused")
        assert has("hiecoatten/fused", "multi_copy") and has("hiecoatten/staged", "bgemm")
        assert has("attentionnet", "dropout") and has("ibowimg", "dropout")
    for coatt in ("parallel", "alternating"):
        b = "ladder/%s/q_length" % coatt
        if b not in logs:
            continue
        for other in ("no_q_length", "masks", "eval", "index", "pair", "packed"):
            differ("ladder/%s/%s" % (coatt, other), b)
        differ("ladder/%s/packed/masks" % coatt, "ladder/%s/packed" % coatt)
        assert logs["ladder/%s/eval/masks-ignored" % coatt] == logs["ladder/%s/eval" % coatt], "the ladder ignores masks in eval"
        assert has("ladder/%s/packed" % coatt, "tanh_dropout_unpack_fwd")
        assert has("ladder/%s/masks" % coatt, "dropout", ":uint8:")
    if "ladder/alternating/packed-coatt" in logs:
        assert has("ladder/alternating/packed-coatt", "tanh_dropout_packed_fwd") and has("ladder/alternating/q_length", "guided_logits_fwd")
        differ("ladder/alternating/packed-coatt/masks", "ladder/alternating/packed-coatt")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="the fingerprint (default: stdout)")
    ap.add_argument("--log", default=None, help="also write every case's call log here")
    ap.add_argument("--only", default=None, help="run the cases whose name contains this")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the fingerprint needs the GPU"
    vqa.lib.load()
    _install_proxy()
    out, full, logs = [], [], {}
    for name, build, switches in _cases():
        if args.only and args.only not in name:
            continue
        log, lines, detail = run_case(name, build, switches)
        logs[name] = log
        out.append("== %s: %d calls, log sha256 %s" % (name, len(log), hashlib.sha256("\n".join(log).encode()).hexdigest()))
        out.append("   " + " ".join("%s=%d" % kv for kv in sorted(_names(log).items())))
        out.extend("   " + l for l in lines)
        full.append("== %s" % name)
        full.extend(log)
        full.extend(detail)
        print("%-50s %5d calls" % (name, len(log)), file=sys.stderr, flush=True)
    if not args.only:
        _check_branches(logs)
        out.append("== branches: every branch the cases name was taken (%d cases)" % len(logs))
    text = "\n".join(out) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(full) + "\n")


if __name__ == "__main__":
    main()
