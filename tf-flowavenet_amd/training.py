"""Training side of the path (train.py:35-83).

``GradEngine`` computes loss = -(log_p + logdet) and its gradient with respect to every trainable
tensor of the reference, ``Trainer`` adds the data-parallel clip / Adam step of ``optim.py``.  The
building blocks are thin wrappers over ``csrc/train_kernels.hip``: ``fwn_gemm`` (generic multi-segment
GEMM on the LDS-DMA ring core: data gradients on transposed packed weights), ``fwn_transpose_shift`` +
split-K ``fwn_tn_gemm_group`` + ``fwn_wn_backward_group`` (weight gradients: K = rows, partials summed in a fixed
order), and the element-wise ``fwn_*_bwd`` kernels.  The sequencing is Python; every activation-sized
arithmetic step runs in ``libfwn.so`` and there is no fallback path.
"""
from __future__ import annotations

import ctypes as C

from . import _lib


_STREAMS = {}     # device -> stream handle, only while a GradEngine call is running (it never switches streams)


def _stream(t):
    import torch
    h = _STREAMS.get(t.device)
    return h if h is not None else torch.cuda.current_stream(t.device).cuda_stream


def gemm(segs, w, n, m, *, ti=0, bias=None, res=None, rscale=1.0, mask=None, relu=False, oscale=1.0,
         out=None, out_f32=False, accumulate=False, nsplit=1, split_stride=0, gate=None, row_len=None):
    """``out[m, n] = oscale * relu?(mask?(sum_s shift(x_s)[:, :k_s] @ w[:, koff_s:koff_s+k_s].T + bias + rscale*res))``.

    segs: list of ``(x, k, shift, koff)`` with ``x`` a bf16 2-D tensor (rows, ld); ``w`` bf16 (n, ldw).
    gate: ``(aux, dpre, col0)`` - the 256 output columns from ``col0`` go through the gate derivative into ``dpre``
    (bf16 [m, 512]) instead of ``out`` (fwn.h ``fwn_gemm_desc.gate_aux``).
    row_len: ``(lengths, samples_per_row)`` with ``lengths`` an int32 device tensor [m / ti] - a ragged batch: the output rows
    past each clip's end are stored as exact 0 (fwn.h ``fwn_gemm_desc.row_len``; refused together with ``accumulate``)."""
    import torch
    lib = _lib.load()
    d = _lib.GemmDesc()
    if not 1 <= len(segs) <= _lib.FWN_GEMM_MAXSEG:
        raise ValueError("1..%d segments" % _lib.FWN_GEMM_MAXSEG)
    for i, (x, k, shift, koff) in enumerate(segs):
        if x.dtype != torch.bfloat16 or x.dim() != 2 or x.stride(1) != 1:
            raise ValueError("segment %d must be a row-major bf16 matrix" % i)
        s = d.seg[i]
        s.x, s.rows, s.ld, s.k, s.shift, s.koff = x.data_ptr(), int(x.shape[0]), int(x.stride(0)), int(k), int(shift), int(koff)
    d.nseg, d.M, d.N, d.Ti = len(segs), int(m), int(n), int(ti)
    d.W, d.ldw = w.data_ptr(), int(w.stride(0))
    d.bias = bias.data_ptr() if bias is not None else None
    if res is not None:
        d.R, d.ldr, d.rscale = res.data_ptr(), int(res.stride(0)), float(rscale)
    if mask is not None:
        d.mask, d.ldmask = mask.data_ptr(), int(mask.stride(0))
    d.relu, d.oscale = int(bool(relu)), float(oscale)
    if out is None:
        shape = (nsplit, m, n) if nsplit > 1 else (m, n)
        out = torch.empty(*shape, dtype=torch.float32 if out_f32 else torch.bfloat16, device=w.device)
    d.Y, d.ldy = out.data_ptr(), int(out.stride(-2))
    d.out_f32, d.accumulate, d.nsplit = int(out.dtype == torch.float32), int(bool(accumulate)), int(nsplit)
    d.split_stride = int(split_stride or (out.stride(0) if nsplit > 1 else 0))
    if gate is not None:
        aux, dpre, col0 = gate
        if aux.dtype != torch.bfloat16 or dpre.dtype != torch.bfloat16 or tuple(aux.shape) != (m, 512) or tuple(dpre.shape) != (m, 512) \
                or not (aux.is_contiguous() and dpre.is_contiguous()):
            raise ValueError("gate: aux and dpre must be contiguous bf16 (m, 512)")
        d.gate_aux, d.gate_out, d.gate_col0 = aux.data_ptr(), dpre.data_ptr(), int(col0)
    if row_len is not None:
        lens, spr = row_len
        if lens.dtype != torch.int32 or not lens.is_contiguous() or ti <= 0 or lens.numel() * ti != m:
            raise ValueError("row_len: a contiguous int32 tensor of m / ti lengths (ti > 0)")
        d.row_len, d.len_spr = lens.data_ptr(), int(spr)
    _lib.check(lib.fwn_gemm(C.byref(d), _stream(w)), "fwn_gemm")
    return out


def transpose_shift(x, m, c, *, shift=0, dshift=0, ntap=1, ti=0, ones_row=False, ld_dst=None):
    """``dst[z*c + c', m'] = x[m' + shift + z*dshift, c']`` for tap z < ntap (zero where the tap leaves its
    clip), bf16 ``[ntap*c (+1), ld_dst]``; ones_row appends a row of ones (for m' < m)."""
    import torch
    lib = _lib.load()
    ld_dst = ld_dst or (m + 63) // 64 * 64
    dst = torch.empty(ntap * c + (1 if ones_row else 0), ld_dst, dtype=torch.bfloat16, device=x.device)
    _lib.check(lib.fwn_transpose_shift(x.data_ptr(), int(m), int(c), int(x.stride(0)), int(shift), int(dshift), int(ntap),
                                       int(ti), dst.data_ptr(), int(ld_dst), int(bool(ones_row)), _stream(x)), "fwn_transpose_shift")
    return dst


def reduce_splits(partial, scale=1.0):
    """``partial [S, ...] fp32 -> sum over S`` in a fixed order (the deterministic second pass of split-K)."""
    import torch
    lib = _lib.load()
    s = int(partial.shape[0])
    out = torch.empty(partial.shape[1:], dtype=torch.float32, device=partial.device)
    _lib.check(lib.fwn_reduce_splits(partial.data_ptr(), s, int(partial.stride(0)), out.numel(), float(scale),
                                     out.data_ptr(), _stream(partial)), "fwn_reduce_splits")
    return out


def weight_grad_partials(x, m, kx, dyt, n, *, shifts=(0,), ti=0, nsplit=None):
    """Split-K partials of ``dW[tap*kx + i, j] = sum_r x[r + shift_tap, i] * dy[r, j]`` with the bias
    gradient ``sum_r dy[r, j]`` as one more row: fp32 ``[S, len(shifts)*kx + 1, n]``.

    x: bf16 [m, >=kx]; dyt: ``transpose_shift(dy, m, n)`` (shared by every weight gradient that
    contracts with the same dy); shifts: an arithmetic progression."""
    mp = int(dyt.shape[1])
    rows = len(shifts) * kx
    dshift = shifts[1] - shifts[0] if len(shifts) > 1 else 0
    xt = transpose_shift(x, m, kx, shift=shifts[0], dshift=dshift, ntap=len(shifts), ti=ti, ones_row=True, ld_dst=mp)
    if nsplit is None:
        nchunks, n128 = mp // 64, (n + 127) // 128
        t256 = ((rows + 1 + 255) // 256) * n128
        if rows + 1 >= 512 and nchunks >= 64:      # long contraction: enough splits for the 256 x 128 tile to fill the chip
            nsplit = max(1, min(nchunks // 8, -(-200 // t256)))
        else:
            nsplit = max(1, min(nchunks, -(-256 // (((rows + 1 + 63) // 64) * n128))))
    part = gemm([(xt, mp, 0, 0)], dyt, n, rows + 1, out_f32=True, nsplit=nsplit)
    return part if nsplit > 1 else part[None]


def tn_weight_grad_partials(x, dy, m, kx, n, *, shifts=(0,), ti=0, nsplit=None, bias_row=True):
    """The same partials (bias row = column sums of dy, last) straight from x and dy as they lie in memory
    (``fwn_tn_gemm``: operands read transposed out of LDS): fp32 ``[S, len(shifts)*kx (+ 1), n]``.
    Needs 16-byte aligned rows: kx, n and both row strides multiples of 8."""
    import torch
    lib = _lib.load()
    rows = len(shifts) * kx
    dshift = shifts[1] - shifts[0] if len(shifts) > 1 else 0
    if nsplit is None:
        tiles = len(shifts) * ((kx + 127) // 128) * ((n + 127) // 128)
        nsplit = max(1, min((m + 63) // 64 // 4 or 1, -(-256 // tiles)))
    part = torch.empty(nsplit, rows + (1 if bias_row else 0), n, dtype=torch.float32, device=x.device)
    _lib.check(lib.fwn_tn_gemm(x.data_ptr(), int(x.stride(0)), int(kx), len(shifts), int(shifts[0]), int(dshift),
                               dy.data_ptr(), int(dy.stride(0)), int(n), int(m), int(ti), int(nsplit), part.data_ptr(),
                               int(part.stride(0)), int(bool(bias_row)), _stream(x)), "fwn_tn_gemm")
    return part


def tn_group_splits(specs, m):
    """Splits of the row range for a group of weight-gradient GEMMs ``(kx, n, ntap)``: as many as keep the whole
    group within ONE round of workgroups (a workgroup per CU), so every GEMM writes few partials."""
    e = int(_lib.load().fwn_tn_gemm_tile(int(m)))             # 128 x 128 or 256 x 256 output tiles at this m
    tiles = sum(ntap * ((kx + e - 1) // e) * ((n + e - 1) // e) for kx, n, ntap in specs)
    return max(1, min((m + 63) // 64, 256 // max(1, tiles)))


def tn_block_splits(specs, n_flow, m):
    """The split count ``fwn_train_loss_and_grads`` uses for the weight-gradient GEMMs ``specs`` of ONE flow: planned for the
    flow's block (csrc/train_api.hip ``tn_block_splits``) - the groups of all ``n_flow`` flows of a block run as one launch
    on the side stream, so a handful of splits fills the chip."""
    e = int(_lib.load().fwn_tn_gemm_tile(int(m)))
    tiles = n_flow * sum(ntap * ((kx + e - 1) // e) * ((n + e - 1) // e) for kx, n, ntap in specs)
    if m < 4096:                            # few rows: bound by writing the output tiles - one split
        return 1
    a = min((m + 63) // 64, 32)
    for n in range(1, a + 1):               # the fewest splits that fill the launch's rounds of 256 workgroups to 85 %
        w = tiles * n
        if 100 * w >= 85 * 256 * ((w + 255) // 256):
            return n
    return max(1, a)


def tn_weight_grad_group(jobs, m, ti=0, nsplit=None):
    """``jobs``: list of ``(x, dy, kx, n, shifts)`` sharing m and ti.  One launch (``fwn_tn_gemm_group``); returns the
    fp32 partials ``[S, len(shifts)*kx + 1, n]`` of every job (views of one buffer; last row = bias gradient)."""
    import torch
    lib = _lib.load()
    if len(jobs) > _lib.FWN_MAX_GROUP:
        return (tn_weight_grad_group(jobs[:_lib.FWN_MAX_GROUP], m, ti, nsplit) +
                tn_weight_grad_group(jobs[_lib.FWN_MAX_GROUP:], m, ti, nsplit))
    if nsplit is None:
        nsplit = tn_group_splits([(kx, n, len(sh)) for _, _, kx, n, sh in jobs], m)
    sizes = [(len(sh) * kx + 1) * n for _, _, kx, n, sh in jobs]
    buf = torch.empty(nsplit * sum(sizes), dtype=torch.float32, device=jobs[0][0].device)
    arr = (_lib.TnJob * len(jobs))()
    parts, off = [], 0
    for q, (x, dy, kx, n, sh), size in zip(arr, jobs, sizes):
        part = buf[off:off + nsplit * size].view(nsplit, len(sh) * kx + 1, n)
        off += nsplit * size
        parts.append(part)
        q.x, q.dy, q.part, q.split_stride = x.data_ptr(), dy.data_ptr(), part.data_ptr(), size
        q.ldx, q.Kx, q.ntap, q.shift0 = int(x.stride(0)), int(kx), len(sh), int(sh[0])
        q.dshift = int(sh[1] - sh[0]) if len(sh) > 1 else 0
        q.ldy, q.N, q.nsplit, q.bias_row = int(dy.stride(0)), int(n), int(nsplit), 1
    _lib.check(lib.fwn_tn_gemm_group(arr, len(jobs), int(m), int(ti), _stream(jobs[0][0])), "fwn_tn_gemm_group")
    return parts


def wn_backward_group(jobs):
    """``jobs``: list of dicts(part [S, rows, ldp], k, n, col0, bias_row (-1: none), scale, row_src, v, g, dv, dg, db):
    split reduction + weight-norm backward of all of them in two launches (``fwn_wn_backward_group``)."""
    import torch
    lib = _lib.load()
    for i0 in range(0, len(jobs), _lib.FWN_MAX_GROUP):
        chunk = jobs[i0:i0 + _lib.FWN_MAX_GROUP]
        arr = (_lib.WnJob * len(chunk))()
        for q, j in zip(arr, chunk):
            part = j["part"]
            q.part, q.split_stride, q.nsplit, q.ldp = part.data_ptr(), int(part.stride(0)), int(part.shape[0]), int(part.shape[2])
            q.row_src = j["row_src"].data_ptr() if j.get("row_src") is not None else None
            q.col_src = j["col_src"].data_ptr() if j.get("col_src") is not None else None
            q.col0, q.bias_row, q.K, q.N, q.scale = int(j.get("col0", 0)), int(j.get("bias_row", -1)), int(j["k"]), int(j["n"]), float(j.get("scale", 1.0))
            q.V = j["v"].data_ptr() if j.get("v") is not None else None
            q.g = j["g"].data_ptr() if j.get("g") is not None else None
            q.dV, q.dg = j["dv"].data_ptr(), j["dg"].data_ptr() if j.get("dg") is not None else None
            q.db = j["db"].data_ptr() if j.get("db") is not None else None
        scr = torch.empty(int(lib.fwn_wn_group_scratch(arr, len(chunk))), dtype=torch.float64, device=chunk[0]["part"].device)
        _lib.check(lib.fwn_wn_backward_group(arr, len(chunk), scr.data_ptr(), _stream(chunk[0]["part"])), "fwn_wn_backward_group")


def colsum_bf16(dy, m, n, scale=1.0, out=None):
    """``out[j] = scale * sum_r dy[r, j]`` (bias gradient), fp32 [n], fixed summation order."""
    import torch
    lib = _lib.load()
    out = torch.empty(n, dtype=torch.float32, device=dy.device) if out is None else out
    scr = torch.empty(lib.fwn_colsum_partials(m, n), dtype=torch.float32, device=dy.device)
    _lib.check(lib.fwn_colsum_bf16(dy.data_ptr(), int(m), int(n), int(dy.stride(0)), float(scale), scr.data_ptr(),
                                   out.data_ptr(), _stream(dy)), "fwn_colsum_bf16")
    return out


def weight_grad(x, dy, m, kx, n, *, shifts=(0,), ti=0, nsplit=None):
    """``(dW [len(shifts)*kx, n], db [n])`` fp32: the partials of ``weight_grad_partials`` summed in a fixed order."""
    dyt = transpose_shift(dy, m, n)
    part = weight_grad_partials(x, m, kx, dyt, n, shifts=shifts, ti=ti, nsplit=nsplit)
    full = reduce_splits(part) if part.shape[0] > 1 else part[0]
    rows = len(shifts) * kx
    return full[:rows], full[rows]


# =============================================================================================
# Loss and gradients of the whole model (train.py:56-66: loss = -(log_p + logdet)): ONE C call per batch,
# fwn_train_loss_and_grads (csrc/train_api.hip sequences the training forward and the backward over the stage
# kernels).  What stays here is parameter-side: the packed bf16 copies the GEMMs read (_TrainPack, refreshed from the
# fp32 masters every step by one gather and the grouped packing launches) and the descriptors that tell the C side where masters,
# copies and gradients live.
# =============================================================================================
import numpy as np

from . import packing, weights

SQH = float(np.sqrt(0.5))


class _TrainPack:
    """Inference packing plus the natural-order / transposed bf16 copies the backward GEMMs read, all recorded into
    one ``packing.PackPlan`` over the flat fp32 masters and refreshed from them every step."""

    def __init__(self, params, hp, device):
        import torch
        self.hp, self.dev = hp, torch.device(device)
        if self.dev.type == "cuda" and self.dev.index is None:      # "cuda" != "cuda:0" for torch: make it concrete
            self.dev = torch.device("cuda", torch.cuda.current_device())
        self.lib = _lib.load()
        self.params = params
        self.pm = packing.pack_model(params, hp, self.dev, cond_mode=1, refresh=True)
        self.plan = self.pm.plan
        self.flows = {}
        self.br = [self._i64(("br", i), packing.bitrev_table(i)) for i in range(hp.n_block)]
        half_ = hp.num_mels // 2
        # logical row of a weight gradient -> row of the GEMM that computed it in device channel order
        self.cond_rows = [self._i32(("cond_rows", i), np.argsort(packing.cond_src_k(i, half_)[:half_ * (2 << i)]))
                          for i in range(hp.n_block)]
        # logical row tap Ch + c of a front weight gradient -> row of the TN GEMM over y_a rows padded to max(Ch, 8) channels
        self.front_rows = [self._i32(("front_rows8", i), np.concatenate([tap * max(1 << i, 8) + packing.bitrev_table(i) for tap in range(3)]))
                           for i in range(hp.n_block)]
        self.csrc64 = [self._i64(("csrc", i), packing.cond_src_k(i, hp.num_mels // 2)[:(hp.num_mels // 2) * (2 << i)])
                       for i in range(hp.n_block)]
        for i in range(hp.n_block):
            for j in range(hp.n_flow):
                self.flows[(i, j)] = self._pack_flow_plan(i, j)
        self.plan.refresh()

    def refresh(self):
        """The masters changed (an optimiser step): re-pack everything into the same buffers."""
        self.plan.refresh()

    def _pack_flow_plan(self, i, j):
        """The backward's transposed copies as jobs of the plan (transposed packing: no separate transposes) and its
        per-flow tables as gather recipes."""
        import torch
        hp, dev, plan = self.hp, self.dev, self.plan
        ch, half, L = 1 << i, hp.num_mels // 2, hp.n_layer
        cin = half * (2 << i)
        wp = weights.flow_prefix(i, j) + "/WaveNet"
        bz = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=dev)
        id256 = self._i32("id256", np.arange(256))
        taps = [self._i32(("tap256", tap), tap * 256 + np.arange(256)) for tap in range(3)]
        csrc = self._i32(("csrc", i), packing.cond_src_k(i, half))
        br = packing.bitrev_table(i).astype(np.int64)
        fk = packing.front_src_k(i)
        P = self.params

        def job(name, src_k, k_dst, src_n, n_dst, out, col, transposed, weight_norm=True):
            plan.add(P[name + "/kernel"], P[name + "/g"] if weight_norm else None, src_k, src_n, k_dst, n_dst,
                     out.data_ptr() + 2 * col, int(out.stride(0)), 1.0, transposed)

        t = {}
        t["WfT"] = bz(ch, 768)
        for tap in range(3):
            job(wp + "/Conv_front", self._i32(("fk", i, tap), fk[tap * ch:(tap + 1) * ch]), ch, id256, 256, t["WfT"], tap * 256, True)
        t["WdT"], t["WcT"], t["WresT"], t["WskipT"] = [], [], [], []
        for l in range(L):
            rp = "%s/ResBlock_%d" % (wp, l)
            wdt = bz(256, 1536)
            for tap in range(3):
                job(rp + "/Conv_filter", taps[tap], 256, id256, 256, wdt, tap * 512, True)
                job(rp + "/Conv_gate", taps[tap], 256, id256, 256, wdt, tap * 512 + 256, True)
            t["WdT"].append(wdt)
            if l == 0:
                t["WcT_all"] = bz(cin, L * 512)          # the layers side by side: one K = L * 512 GEMM for the conditioning gradient
            wct = t["WcT_all"][:, l * 512:(l + 1) * 512]
            job(rp + "/filter_conv_c", csrc, cin, id256, 256, wct, 0, True)
            job(rp + "/gate_conv_c", csrc, cin, id256, 256, wct, 256, True)
            t["WcT"].append(wct)
            if l + 1 < L:
                wrt = bz(256, 256)
                job(rp + "/res_conv", id256, 256, id256, 256, wrt, 0, True)
                t["WresT"].append(wrt)
            if l == 0:
                t["WskipT_all"] = bz(L * 256, 256)              # the L transposed skip convs stacked along N: one GEMM for all do_l
            wst = t["WskipT_all"][l * 256:(l + 1) * 256]
            job(rp + "/skip_conv", id256, 256, id256, 256, wst, 0, True)
            t["WskipT"].append(wst)
        # (the forward half runs the inference tail on the inference packing: no natural-order Wskip / Wfin / Wz copies)
        t["WfinT"] = bz(256, 256)
        job(wp + "/Conv_final", id256, 256, id256, 256, t["WfinT"], 0, True)
        zcol = np.concatenate([br, ch + br])
        t["zcol"] = self._i64(("zcol", i), zcol)
        t["zinv32"] = self._i32(("zinv", i), np.argsort(zcol))
        zc32 = self._i32(("zcol", i), zcol)
        n2 = 2 * ch
        t["ldz"] = max(8, n2)
        t["WzT"] = bz(256, t["ldz"])
        job(wp + "/ZeroConv1d", id256, 256, zc32, n2, t["WzT"], 0, True, weight_norm=False)
        # per-flow bias / scale vectors in device channel order (the backward reads ez), in fp32 with the terms in order
        t["bfin"] = P[wp + "/Conv_final/bias"]
        plan.table(lambda v: t.__setitem__("bskip", v), (256,),
                   dict(terms=[("%s/ResBlock_%d/skip_conv/bias" % (wp, l), np.arange(256)) for l in range(L)], fp32=True))
        plan.table(lambda v: t.__setitem__("bz", v), (n2,), dict(terms=[(wp + "/ZeroConv1d/bias", zcol)], fp32=True))
        plan.table(lambda v: t.__setitem__("ez", v), (n2,), dict(terms=[(wp + "/ZeroConv1d/scale", zcol)], post=3.0, exp=True, fp32=True))
        return t

    def _i32(self, key, arr):
        import torch
        gk = (str(self.dev), self.hp.num_mels, "train", key)
        if gk not in packing._IDX_CACHE:
            packing._IDX_CACHE[gk] = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int32)).to(self.dev)
        return packing._IDX_CACHE[gk]

    def _i64(self, key, arr):
        import torch
        gk = (str(self.dev), self.hp.num_mels, "train64", key)
        if gk not in packing._IDX_CACHE:
            packing._IDX_CACHE[gk] = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int64)).to(self.dev)
        return packing._IDX_CACHE[gk]

    def _f32(self, name):
        """The fp32 device master of parameter ``name`` (a view of the flat vector the plan reads)."""
        return self.params[name]


class DeviceLengths:
    """Lengths of a ragged batch that are already on the device and already validated: an int32 tensor [B] that
    ``GradEngine.loss_and_grads`` hands to the kernels as it is, without reading it on the host (the recorded step's static
    buffer: only kernels read it, at replay)."""

    def __init__(self, tensor):
        self.tensor = tensor


class GradEngine:
    """``loss_and_grads(params, x, c)``: one training forward + backward on the current device.

    params: dict name -> fp32 array / tensor in the reference's layouts (``weights.param_shapes``); views of one flat
    fp32 device vector (the optimiser's masters) are read in place, anything else is copied into a flat vector the
    engine owns, on every call.
    Returns ``(loss, log_p, logdet, grads)`` with grads a dict name -> fp32 device tensor of the
    parameter's shape (``d loss / d param``, loss = -(log_p + logdet), train.py:60).

    ``loss_and_grads(params, x, c, lengths=[...])``: a ragged batch (the rules of ``FloWaveNet.forward(..., lengths=)``).  Clip
    ``b`` is ``x[b, :lengths[b]]`` with ``c[b, :lengths[b] // hop]``; loss = -(1/B) sum_b (log_p[b] + logdet[b]) with every
    clip's scalars taken over its own samples, and each gradient is the mean over the clips of that clip's own gradient -
    whatever (finite) ``x`` and ``c`` hold past a clip's end reaches no bit of either.  log_p / logdet are the batch means;
    ``per_clip`` then holds the fp32 tensors ``(log_p [B], logdet [B])`` of that call (None after a plain call)."""

    def __init__(self, hparams, device="cuda", side_stream=True):
        """side_stream: each block's weight gradients run on a second stream under the next block's backward chain
        (fwn_train_desc.side_stream); False keeps the one-stream sequence, the bit-for-bit reference of the tests."""
        if not hparams.affine or hparams.causality:
            raise NotImplementedError("affine=True, causality=False only")
        self.hp, self.device = hparams, device
        self.lib = _lib.load()
        self._gout = None
        self._on_block = None
        self._own_flat = None
        self.side_stream = bool(side_stream)
        self._side = None
        self.per_clip = None

    # ------------------------------------------------------------------ helpers
    def _side_stream(self, dev):
        """The second stream of a step, or None without one."""
        import torch
        if not self.side_stream:
            return None
        if self._side is None:            # an engine serves one device
            self._side = torch.cuda.Stream(torch.device(dev))
        return self._side

    def _call(self, name, *args):
        _lib.check(getattr(self.lib, name)(*args), name)

    def loss_and_grads(self, params, x, c, grad_out=None, on_block_done=None, lengths=None, repack=True):
        """grad_out: optional dict name -> fp32 tensor (e.g. views of a flat gradient buffer): gradients are
        written there (the large ones in place) and returned as those very tensors.  on_block_done(i) is
        called when every gradient of block i is in grad_out (blocks finish last to first; -1 = the
        up-sampling convs, at the end) - the hook a data-parallel step uses to start that block's
        all-reduce under the rest of the backward pass.
        lengths: a list, NumPy array or tensor of B sample counts (a ragged batch, see the class) - validated on the host
        by ``model.check_lengths`` before anything is launched; or ``DeviceLengths`` (already validated, read at run time).
        repack: False skips the re-pack of the bf16 copies from the fp32 masters - for a caller that knows the masters have not
        moved since this engine's last call on them (the later micro-batches of a gradient accumulation); the first call on a
        set of masters packs whatever it says."""
        self._gout = grad_out
        self._on_block = on_block_done
        try:
            return self._loss_and_grads(params, x, c, lengths, repack)
        finally:
            _STREAMS.clear()
            self._gout = None
            self._on_block = None

    def check_lengths(self, lengths, b, t):
        """The host-side validation of a ragged batch: ``FloWaveNet``'s own (``model.check_lengths``) -> list of B ints."""
        from . import model
        if getattr(self.hp, "gate_fp8", False):
            raise ValueError("gate_fp8 hparams take no lengths: the e4m3 copies of h are not masked")
        return model.check_lengths(lengths, b, t, int(np.prod(self.hp.upsample_scales)), self.hp.n_block)

    def _loss_and_grads(self, params, x, c, lengths=None, repack=True):
        import torch
        hp, lib = self.hp, self.lib
        dev = torch.device(self.device)
        if lengths is not None and not isinstance(lengths, DeviceLengths):      # validated on the host before anything is launched
            shape = tuple(torch.as_tensor(x).shape)
            b_ = int(shape[0]) if shape else 0
            lengths = self.check_lengths(lengths, b_, int(np.prod(shape[1:])) if shape else 0)
        st = torch.cuda.current_stream(dev).cuda_stream
        _STREAMS.clear()
        _STREAMS[torch.zeros(0, device=dev).device] = st
        shp = self._shapes = weights.param_shapes(hp)
        if not weights.is_flat(params, dev):
            if self._own_flat is None:
                self._own_flat = torch.zeros(weights.FlatLayout(hp).size, dtype=torch.float32, device=dev)
            params = weights.flat_views(params, hp, dev, out=self._own_flat)
        key = next(iter(params.values())).data_ptr()
        tp = getattr(self, "_tp", None)
        if tp is not None and getattr(self, "_tp_key", None) == key:
            if repack:
                tp.refresh()
        else:
            tp = self._tp = _TrainPack(params, hp, self.device)
            self._tp_key = key
        x = torch.as_tensor(x).to(device=dev, dtype=torch.float32).contiguous()
        c = torch.as_tensor(c).to(device=dev, dtype=torch.float32).contiguous()
        B, T = int(x.shape[0]), int(x.shape[1])
        if T % (1 << hp.n_block) or int(c.shape[1]) * hp.hop_size != T:
            raise ValueError("bad shapes")
        lens = None
        if isinstance(lengths, DeviceLengths):
            lens = lengths.tensor
            if lens.dtype != torch.int32 or lens.device != x.device or tuple(lens.shape) != (B,) or not lens.is_contiguous():
                raise ValueError("DeviceLengths must hold a contiguous int32 tensor [B=%d] on %s" % (B, x.device))
        elif lengths is not None:
            lens = torch.tensor(lengths, dtype=torch.int32).to(dev)
        return self._run(tp, params, x.reshape(B, T), c, B, T, st, lens)

    def _run(self, tp, params, x, c, B, T, st, lens=None):
        """One call of ``fwn_train_loss_and_grads`` (csrc/train_api.hip sequences forward and backward): this method only
        fills the descriptors - packed copies, masters, gradient destinations, per-step tables - and lends a workspace."""
        import torch
        hp, lib, dev = self.hp, self.lib, x.device
        L = hp.n_layer
        shp = self._shapes
        go = self._gout
        if go is None:          # no caller-owned gradient buffers: one fresh contiguous tensor per parameter
            go = {k: torch.empty(v, dtype=torch.float32, device=dev) for k, v in shp.items()}
        elif not all(go[k].is_contiguous() for k in shp):
            raise ValueError("grad_out tensors must be contiguous")
        masters = {k: tp._f32(k) for k in shp}
        ptr = lambda t_: t_.data_ptr() if t_ is not None else None
        key = (tuple(masters[k].data_ptr() for k in shp), tuple(go[k].data_ptr() for k in shp))
        if getattr(self, "_desc_key", None) != key:
            nfl = hp.n_block * hp.n_flow
            flows = (_lib.FlowTrainDesc * nfl)()
            td = _lib.TrainDesc()
            keep = []

            def conv(cg, name, weight_norm=True):
                cg.V, cg.dV, cg.db = ptr(masters[name + "/kernel"]), ptr(go[name + "/kernel"]), ptr(go[name + "/bias"])
                if weight_norm:
                    cg.g, cg.dg = ptr(masters[name + "/g"]), ptr(go[name + "/g"])

            for i in range(hp.n_block):
                for j in range(hp.n_flow):
                    f, t = flows[i * hp.n_flow + j], tp.flows[(i, j)]
                    fp = weights.flow_prefix(i, j)
                    wp = fp + "/WaveNet"
                    f.WfT, f.WskipT_all = ptr(t["WfT"]), ptr(t["WskipT_all"])
                    f.WfinT, f.WzT, f.ldz = ptr(t["WfinT"]), ptr(t["WzT"]), int(t["ldz"])
                    f.wct_ld = int(t["WcT_all"].stride(0))
                    for l in range(L):
                        rp = "%s/ResBlock_%d" % (wp, l)
                        f.WdT[l], f.WcT[l] = ptr(t["WdT"][l]), ptr(t["WcT"][l])
                        if l + 1 < L:
                            f.WresT[l] = ptr(t["WresT"][l])
                        conv(f.filt[l], rp + "/Conv_filter"); conv(f.gate[l], rp + "/Conv_gate")
                        conv(f.res[l], rp + "/res_conv"); conv(f.skip[l], rp + "/skip_conv")
                        conv(f.filt_c[l], rp + "/filter_conv_c"); conv(f.gate_c[l], rp + "/gate_conv_c")
                    conv(f.front, wp + "/Conv_front"); conv(f.final_, wp + "/Conv_final"); conv(f.zero, wp + "/ZeroConv1d", weight_norm=False)
                    f.d_an_b, f.d_an_logs = ptr(go[fp + "/ActNorm/b"]), ptr(go[fp + "/ActNorm/logs"])
                    f.d_zscale = ptr(go[wp + "/ZeroConv1d/scale"])
                td.cond_rows[i], td.front_rows[i] = ptr(tp.cond_rows[i]), ptr(tp.front_rows[i])
                td.zinv32[i], td.br[i] = ptr(tp.flows[(i, 0)]["zinv32"]), ptr(tp.br[i])
                td.zcol[i] = ptr(tp.flows[(i, 0)]["zcol"])
            for n in range(len(hp.upsample_scales)):
                td.up_bias_dev[n] = ptr(masters["upsample_%d/bias" % n])
                u = td.up[n]
                u.V, u.g = ptr(masters["upsample_%d/kernel" % n]), ptr(masters["upsample_%d/g" % n])
                u.dV, u.dg, u.db = ptr(go["upsample_%d/kernel" % n]), ptr(go["upsample_%d/g" % n]), ptr(go["upsample_%d/bias" % n])
            td.model = C.pointer(tp.pm.model_desc)
            td.flows = C.cast(flows, C.POINTER(_lib.FlowTrainDesc))
            td.zero_dead_res = 1            # first call on these gradient buffers: the dead res_conv gradients are zeroed once
            self._desc, self._desc_flows, self._desc_key = td, flows, key
        else:
            td, flows = self._desc, self._desc_flows
        # per-step tables (recomputed from the masters before every step: their addresses may move)
        for i in range(hp.n_block):
            for j in range(hp.n_flow):
                f, t = flows[i * hp.n_flow + j], tp.flows[(i, j)]
                tabs = [t[k] if t[k].is_contiguous() else t[k].contiguous() for k in ("bskip", "bfin", "bz", "ez")]
                f.bskip, f.bfin, f.bz, f.ez = (x_.data_ptr() for x_ in tabs)
                t["_tabs_alive"] = tabs
        # the weight gradients of a block run on a second stream under the next block's chain (fwn.h fwn_train_desc.side_stream)
        side = self._side_stream(dev)
        td.side_stream = side.cuda_stream if side is not None else None
        wkey = (B, T, str(dev), bool(td.side_stream), lens is not None)
        if getattr(self, "_ws_key", None) != wkey:
            wname = "fwn_train_ragged_workspace_bytes" if lens is not None else "fwn_train_workspace_bytes"
            need = int(getattr(lib, wname)(C.byref(td), B, T))
            if need == 0:
                _lib.check(-1, wname)
            self._ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
            self._ws_key = wkey
        ws = self._ws
        off = (-ws.data_ptr()) % 256
        out3 = torch.empty(3, dtype=torch.float32, device=dev)
        hook, failure = self._on_block, []

        def block_done(user, blk):
            # ctypes prints and DROPS an exception raised inside a callback: a failed all-reduce or graph cut would go
            # unnoticed and the optimiser would step on un-reduced gradients.  Catch it, make the C sequencer stop
            # (non-zero return) and re-raise once the call is back.
            try:
                if hook is not None:
                    hook(blk)
                return 0
            except BaseException as e:
                failure.append(e)
                return 1

        cb = _lib.BLOCK_DONE_FN(block_done)
        if lens is None:
            self.per_clip = None
            rc = lib.fwn_train_loss_and_grads(C.byref(td), B, T, x.data_ptr(), c.data_ptr(), ws.data_ptr() + off, ws.numel() - off,
                                              out3.data_ptr(), cb, None, st)
        else:
            out2b = torch.empty(2, B, dtype=torch.float32, device=dev)
            self.per_clip = (out2b[0], out2b[1])
            rc = lib.fwn_train_loss_and_grads_ragged(C.byref(td), B, T, x.data_ptr(), c.data_ptr(), lens.data_ptr(), ws.data_ptr() + off,
                                                     ws.numel() - off, out3.data_ptr(), out2b.data_ptr(), cb, None, st)
        if failure:
            raise failure[0]
        _lib.check(rc, "fwn_train_loss_and_grads_ragged" if lens is not None else "fwn_train_loss_and_grads")
        td.zero_dead_res = 0
        self._alive = (masters, x, c, lens)     # until the stream has consumed them
        return out3[0], out3[1], out3[2], {k: go[k] for k in shp}


class Trainer:
    """One rank of the data-parallel training step (train.py:35-83 ``build_model`` + the session loop
    body): gradients of -(log_p + logdet) on this rank's batch (``GradEngine``), then
    ``optim.DataParallelAdam`` = RCCL all-reduce of the flat gradient, global-norm clip, Adam on the
    fp32 masters.  ``ddi`` performs the ActNorm data-dependent init of the first step
    (train.py:221,229 with init=True)."""

    def __init__(self, hparams, params, device="cuda", group=None, graph=True):
        """graph: record the step into hipGraphs after one eager step per input shape and replay it from then on
        (the step is ~5700 launches; replaying removes their host cost)."""
        from .optim import DataParallelAdam
        self.hp, self.device = hparams, device
        self.opt = DataParallelAdam(hparams, params, device, group=group, grad_reduce_dtype=getattr(hparams, "grad_reduce_dtype", "fp32"),
                                    exchange=getattr(hparams, "grad_exchange", "allreduce"))
        self.engine = GradEngine(hparams, device)
        self.graph = bool(graph)
        self._recorded = {}
        self._recorded_acc = {}     # the recordings only a gradient accumulation makes: (shape key, kind) -> as _recorded
        self.pending = 0            # micro-batches accumulated since the last update (accumulate)
        self._sums = self._pending_b = None
        self.per_clip = None
        # False: skip the gradient exchange (bench.py's compute-only step time, to price the overlap)
        self.exchange = True

    def ddi(self, x, c, lengths=None):
        """ActNorm data-dependent init from the GLOBAL batch (train.py:221,229 with init=True): each rank pushes its
        shard through the flows and the per-channel moments are all-reduced flow by flow (``FloWaveNet`` with
        ``group``), so every rank derives bit-identical b / logs - the single-process result on the concatenated
        batch up to summation order.  (The reference lets its towers race on this assign: SURVEY section 2.1 C2.)
        lengths: a ragged batch (``FloWaveNet.forward_init``) - the statistics are those of the clips' own rows, and the ranks
        are weighted by the rows they hold."""
        from .model import FloWaveNet
        import torch
        views = self.opt.master_views()
        m = FloWaveNet(self.hp, init=True, device=self.device, cond_mode=1, group=self.opt.group).load_params(views)
        xx = torch.as_tensor(x).to(self.device)
        if isinstance(lengths, DeviceLengths):      # the init runs once and validates on the host: read them back
            lengths = lengths.tensor.cpu().tolist()
        if lengths is not None:
            m.forward_init(xx.reshape(xx.shape[0], -1, 1), torch.as_tensor(c).to(self.device), lengths)
        else:
            m.forward(xx.reshape(xx.shape[0], -1, 1), torch.as_tensor(c).to(self.device))
        for k, v in m.export_actnorm().items():
            views[k].copy_(torch.as_tensor(v).to(self.device).reshape(views[k].shape))
        # Only the ActNorm tables were made identical above (moment all-reduce).  Any other per-rank difference in the
        # initial masters - caller-supplied params, another seed, a restore that went differently - would survive every
        # all-reduced step: check once, here, that the ranks start in lock-step.
        if not self.opt.weights_identical():
            raise RuntimeError("Trainer.ddi: the ranks hold different master weights after the data-dependent init "
                               "(different initial parameters or checkpoints per rank?)")

    def step(self, x, c, lengths=None):
        """-> (loss, log_p, logdet, grad_norm) device scalars; the masters are updated in place.
        lengths: a ragged batch (``GradEngine.loss_and_grads``): loss, log_p and logdet are then the means over the clips of
        the per-clip values, which ``per_clip`` holds afterwards as ``(log_p [B], logdet [B])`` (None after a plain step).
        The recorded step keeps the lengths in a static device buffer beside x and c - one recording per shape serves every
        batch, whatever its lengths.  ``lengths=DeviceLengths(t)``: an int32 device tensor [B] of lengths that are legal by
        construction (``corpus.DeviceCorpus.draw``) - nothing is validated or read on the host, the recorded step copies them
        device to device; ``accumulate`` and ``ddi`` take them too (``ddi`` reads them back: it runs once).
        With ``pending`` = n micro-batches accumulated (``accumulate``): this batch is the last of the update.  Its gradient
        takes the pending sum in, block range by block range as the ranges become final - ``opt.g`` = ((g_0 + g_1) + ...) + g_n
        in call order -, then exchange, norm and clip / Adam run as ever with the loss scale n + 1.  loss, log_p and logdet
        are the means over the n + 1 micro-batches (device arithmetic, no host synchronisation), ``per_clip`` is the last
        micro-batch's.  With nothing pending this is the step it always was, to the bit."""
        import torch
        lengths = self._admit(x, lengths)
        n = self.pending
        if self.graph and self.opt.exchange == "allreduce":     # (the sharded exchange is eager only: optim.record_update)
            out = self._step_recorded(x, c, lengths, n=n)
        else:
            out = self._step_eager(x, c, lengths, n=n)
        if not n:
            return out
        mean = (self._sums + torch.stack(out[:3])) / float(n + 1)
        self.drop_pending()
        return mean[0], mean[1], mean[2], out[3]

    def accumulate(self, x, c, lengths=None):
        """-> (loss, log_p, logdet) of this micro-batch; its gradient on the current masters joins the pending sum.  No
        collective, no update, ``global_step`` unchanged: the next ``step`` ends the update (one optimiser update over
        ``pending`` + 1 micro-batches, averaged).  Every micro-batch of an update holds the same number of clips (the mean of
        the means is the mean over the clips only then; ValueError otherwise, before anything is launched and with the pending
        state as it was); T may differ.  The first micro-batch of an update re-packs the bf16 copies from the masters (a restore
        or ``ddi`` may have touched them), the following ones do not: nothing may write the masters between the first
        ``accumulate`` of an update and its ``step``.  Data parallel: every rank must call ``accumulate`` the same number of
        times per update - nothing checks it (a collective would cost what the accumulation saves); ``train.py`` does by
        construction."""
        import torch
        lengths = self._admit(x, lengths)
        first = self.pending == 0
        self.opt.ensure_accumulator()          # outside any recording: the buffer must not come from a graph's pool
        if self.graph and self.opt.exchange == "allreduce":
            out = self._step_recorded(x, c, lengths, micro=first)
        else:
            out = self._micro_eager(x, c, lengths, first)
        cur = torch.stack(out[:3])
        self._sums = cur if first else self._sums + cur
        self._pending_b = int(torch.as_tensor(x).shape[0])
        self.pending += 1
        return cur[0], cur[1], cur[2]

    def drop_pending(self):
        """Forget the pending sum (e.g. after an exception in the middle of an update): the next ``step`` is a plain one."""
        self.pending, self._sums, self._pending_b = 0, None, None

    def _admit(self, x, lengths):
        """What is checked on the host before anything is launched: the lengths of a ragged batch (-> list of ints) and, with
        micro-batches pending, that this one holds as many clips as they did.  ``DeviceLengths`` pass as they are: whoever
        built them (``corpus.DeviceCorpus.draw``) made them legal, and reading them here would cost a synchronisation."""
        import torch
        xs = torch.as_tensor(x)
        b = int(xs.shape[0]) if xs.dim() else 0
        if isinstance(lengths, DeviceLengths):
            if getattr(self.hp, "gate_fp8", False):
                raise ValueError("gate_fp8 hparams take no lengths: the e4m3 copies of h are not masked")
        elif lengths is not None:
            lengths = self.engine.check_lengths(lengths, b, int(xs.numel() // max(1, b)))
        if self.pending and b != self._pending_b:
            raise ValueError("gradient accumulation: this micro-batch holds %d clips, the %d pending ones hold %d each (the mean "
                             "of the micro-batch means is the mean over the clips only for equal sizes)" % (b, self.pending, self._pending_b))
        return lengths

    def _ranges(self):
        return {("upsample" if key == "upsample" else int(key.split("_")[1])): (lo, hi) for key, lo, hi in self.opt.block_ranges()}

    def _step_recorded(self, x, c, lengths=None, n=0, micro=None):
        """First call at a shape: eager (creates the packing plan, fills every cache).  Second: record.  The
        recording is a chain of hipGraphs cut where a block's gradients are final, so that with more than one
        rank each block's all-reduce still starts between two replays, under the rest of the backward pass;
        the Adam rate is refreshed before the replay (the packing, tables included, is inside the recording).
        n: micro-batches pending - the folds of their sum are captured inside the segments, each in front of the cut that
        starts its range's exchange, and the recorded update carries gscale = 1 / (world (n + 1)): a recording per n.
        micro: True / False - not an update but a micro-batch that does not end one, the first of its update (it re-packs and
        starts the sum) or a later one: ONE uncut hipGraph at any world size - gradients and the whole-buffer accumulation, no
        hooks - that returns (loss, log_p, logdet, None)."""
        import torch
        import torch.distributed as dist
        dev = torch.device(self.device)
        x = torch.as_tensor(x)
        c = torch.as_tensor(c)
        # the shapes, not the lengths: one recording serves every ragged batch (the plain step keeps its own key)
        key = (tuple(x.shape), tuple(c.shape)) + (("ragged",) if lengths is not None else ())
        table = self._recorded
        if n or micro is not None:
            table, key = self._recorded_acc, (key, ("micro", bool(micro)) if micro is not None else ("step", n))
        if micro is not None:
            eager = lambda: self._micro_eager(x, c, lengths, micro) + (None,)
        else:
            eager = lambda: self._step_eager(x, c, lengths, n=n)
        rec = table.get(key)
        if rec is None:
            table[key] = "warm"
            return eager()
        ranges = self._ranges()
        world = dist.get_world_size(self.opt.group) if dist.is_available() and dist.is_initialized() else 1
        if rec == "warm":
            # cut(-1) below holds for the side-stream sequence only: one stream enqueues the up-sampling backward between
            # the hooks of block 0 and -1
            if not self.engine.side_stream:
                raise RuntimeError("Trainer: the recorded step needs a GradEngine with side_stream=True")
            xs = torch.empty(tuple(x.shape), dtype=torch.float32, device=dev)
            cs = torch.empty(tuple(c.shape), dtype=torch.float32, device=dev)
            nlen = lengths.tensor.numel() if isinstance(lengths, DeviceLengths) else len(lengths) if lengths is not None else 0
            ls = torch.empty(nlen, dtype=torch.int32, device=dev) if lengths is not None else None
            params, gv = self.opt.master_views(), self.opt.grad_views()
            segs, pool = [], torch.cuda.graph_pool_handle()
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            cur = [None]
            try:
                with torch.cuda.stream(side):
                    cur[0] = torch.cuda.CUDAGraph()
                    # thread_local: other threads (the RCCL watchdog of a data-parallel run polls events) may call
                    # HIP while this thread records
                    cur[0].capture_begin(pool=pool, capture_error_mode="thread_local")

                    def cut(i):
                        if n:       # the pending sum of this range, still inside the segment that ends here
                            self.opt.fold_pending(*ranges["upsample" if i < 0 else i])
                        if world == 1 and i >= 0 and not self.opt.force_collectives:
                            return
                        if i == -1 and not n and segs and segs[-1][1] == 0:     # (with n the up-sampling range's fold lies between)
                            # fwn_train_loss_and_grads reports block 0 and then the up-sampling convs (-1) back to back - with the
                            # side stream block 0 is joined behind the up-sampling backward, nothing is enqueued between the two hooks
                            # (csrc/train_api.hip: join_pending, then the -1 hook) - so there is nothing to cut: no empty
                            # hipGraph segment, only the exchange of the up-sampling range to start
                            segs.append((None, -1))
                            return
                        cur[0].capture_end()
                        segs.append((cur[0], i))
                        cur[0] = torch.cuda.CUDAGraph()
                        cur[0].capture_begin(pool=pool, capture_error_mode="thread_local")

                    loss, log_p, logdet, _ = self.engine.loss_and_grads(params, xs, cs, grad_out=gv, on_block_done=cut if micro is None else None,
                                                                        lengths=DeviceLengths(ls) if ls is not None else None,
                                                                        repack=(n == 0) if micro is None else micro)
                    per_clip = self.engine.per_clip
                    if micro is None:
                        gnorm = self.opt.record_update(loss_scale=n + 1)
                    else:
                        self.opt.accumulate_pending(micro)
                        gnorm = None
                    cur[0].capture_end()
                    segs.append((cur[0], None))
            except Exception as e:      # recording is an optimisation: a runtime that refuses it must not stop training
                import warnings
                try:
                    if cur[0] is not None:
                        cur[0].capture_end()
                except Exception:
                    pass
                torch.cuda.synchronize(dev)
                warnings.warn("recording the training step failed (%s: %s); continuing with eager steps" % (type(e).__name__, e))
                self.graph = False
                return eager()
            torch.cuda.current_stream(dev).wait_stream(side)
            rec = table[key] = dict(xs=xs, cs=cs, ls=ls, segs=segs, out=(loss, log_p, logdet, gnorm), per_clip=per_clip)
        rec["xs"].copy_(x.reshape(rec["xs"].shape), non_blocking=True)
        rec["cs"].copy_(c, non_blocking=True)
        if isinstance(lengths, DeviceLengths):      # already on the device: a copy in stream order, nothing read on the host
            rec["ls"].copy_(lengths.tensor, non_blocking=True)
        elif rec["ls"] is not None:
            rec["ls"].copy_(torch.tensor(lengths, dtype=torch.int32), non_blocking=False)
        self.per_clip = rec["per_clip"]
        if micro is None:
            self.opt.advance()
        works = []
        for g, i in rec["segs"]:
            if i is None:                       # the optimiser: every exchange must have landed
                for w in works:
                    if w is not None:
                        w.wait()
            if g is not None:
                g.replay()
            if i is not None and self.exchange:
                lo, hi = ranges["upsample" if i < 0 else i]
                works.append(self.opt.allreduce_range(lo, hi))
        return rec["out"]

    def _step_eager(self, x, c, lengths=None, n=0):
        params = self.opt.master_views()
        gv = self.opt.grad_views()
        ranges = {("upsample" if key == "upsample" else int(key.split("_")[1])): (lo, hi) for key, lo, hi in self.opt.block_ranges()}
        works = []
        # n micro-batches pending: their sum joins a block's range in front of that range's all-reduce (the ranges cover the
        # layout); the sharded exchange starts no all-reduce here and takes the whole buffer at once below
        fold_ranges = n > 0 and self.opt.exchange != "zero1"

        def block_done(i):      # block i's gradients are final: its all-reduce runs under the remaining backward
            lo, hi = ranges["upsample" if i < 0 else i]
            if fold_ranges:
                self.opt.fold_pending(lo, hi)
            if self.exchange:
                works.append(self.opt.allreduce_range(lo, hi))

        loss, log_p, logdet, grads = self.engine.loss_and_grads(params, x, c, grad_out=gv, on_block_done=block_done, lengths=lengths,
                                                                repack=n == 0)
        self.per_clip = self.engine.per_clip
        if n and not fold_ranges:
            self.opt.fold_pending()
        gnorm = self.opt.step(loss_scale=n + 1, works=works)
        return loss, log_p, logdet, gnorm

    def _micro_eager(self, x, c, lengths, first):
        """A micro-batch that does not end the update: its gradient into ``opt.g`` (no hooks: nothing is exchanged), then into
        the pending sum."""
        loss, log_p, logdet, _ = self.engine.loss_and_grads(self.opt.master_views(), x, c, grad_out=self.opt.grad_views(), lengths=lengths,
                                                            repack=first)
        self.per_clip = self.engine.per_clip
        self.opt.accumulate_pending(first)
        return loss, log_p, logdet
