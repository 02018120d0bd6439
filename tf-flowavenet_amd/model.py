"""``FloWaveNet`` - the reference's model surface (model.py:282-404) on MI355X.

Same class name, constructor arguments, method names, argument order, shapes and
return arity as the reference; torch tensors on a HIP device replace TF tensors
and calls execute eagerly on the current HIP stream.  All arithmetic runs in
``csrc/libfwn.so`` (C ABI in ``include/fwn.h``); there is no fallback path.

Differences that are deliberate (DESIGN.md "Deviations"):
  * ``hparams.dtype`` float16 -> bfloat16 hidden activations / weights with fp32
    accumulation; the flow state, ActNorm, coupling and all reductions stay fp32
    (the reference takes its means in fp16, model.py:135,343);
  * ``reverse`` returns fp32 by default (the flow state is fp32 here); ``reverse(..., dtype="hparams")`` returns
    ``hparams.dtype`` like the reference (model.py:356-357,396);
  * global (speaker) conditioning is inert in the reference (``WaveNet.__call__``
    drops ``g``, modules.py:188-189): ``g`` is validated like the reference does
    (model.py:320-321,353-354) and otherwise ignored;
  * ``affine=False`` / ``causality=True`` are not BASELINE configurations: rejected.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, packing, weights, windowed
from .windowed import ForwardStream, SynthesisStream  # noqa: F401  (the streams' public home is this module)


class FloWaveNet:
    def __init__(self, hparams, init=False, scope="FloWaveNet", device="cuda", cond_mode=0, group=None, gate_fp8=None,
                 persist_mode=None, chain_mode=None, tail_stream=True, cond_stream=True, gate_hs_stream=True):
        """persist_mode (default: ``hparams.persist_mode`` if present, else 0): which small-M flows run as ONE launch
        (csrc/flow_persist.h, ``fwn_model_desc.persist_mode``) - 0: those of up to 512 rows, 1: none, 2: wherever the form
        exists.  chain_mode (``fwn_model_desc.chain_mode``): 0 chains the flows of a block, 1 runs every flow on its own.
        Both select among kernels that compute the same arithmetic; they are arguments of the model, not process variables.
        tail_stream=False leaves the fragment-order copy of Wskip | Wfinal unpacked, so that the tail runs the kernels of
        rounds 2 - 5 everywhere (csrc/tail_chain.h and the N-split ring GEMMs instead of csrc/tail_rs.h): the one-launch flows
        reproduce THOSE bit for bit below 4 097 rows (tests, bench.py's identity check).
        cond_stream=False leaves the fragment-order copy of the hoisted conditioning's weights unpacked (csrc/cond_rs.h): the
        ring-tile kernel then runs at every row count (same sums in the same order, other split counts).
        gate_hs_stream=False leaves the fragment-order copy of the dilated conv's weights unpacked (csrc/cond_rs.h
        gate_hs_kernel): the gates with a hoisted P then run the ring tile at every row count (bit-identical).
        group: the ``torch.distributed`` process group a data-parallel job shards its batch over (None = the
        default group when one is initialised; False: none - a model only one rank builds).  It only matters for ``init=True`` and ``forward_init``: the ActNorm data-dependent
        init then uses the statistics of the GLOBAL batch (moments all-reduced flow by flow) so every rank ends
        with the same parameters - the reference's towers race on that assign (model.py:39, train.py:43-57)."""
        if not hparams.affine:
            raise NotImplementedError("affine=False (additive coupling, model.py:136-139) is out of scope")
        if hparams.causality:
            raise NotImplementedError("causality=True (modules.py:12-13,30-31) is out of scope")
        if hparams.n_block < 1 or hparams.n_flow < 1 or hparams.n_layer < 1:
            raise ValueError("n_block, n_flow and n_layer must be >= 1")
        self._hparams = hparams
        self._scope = scope
        self._init = bool(init)
        self._device = device
        self._cond_mode = cond_mode
        self._group = group
        # fp8 (e4m3) dilated taps where the shape has such a kernel (BASELINE configs[4]); default: hparams.gate_fp8
        self._gate_fp8 = bool(getattr(hparams, "gate_fp8", False) if gate_fp8 is None else gate_fp8)
        self._persist_mode = int(getattr(hparams, "persist_mode", 0) if persist_mode is None else persist_mode)
        self._chain_mode = int(getattr(hparams, "chain_mode", 0) if chain_mode is None else chain_mode)
        if self._persist_mode not in (0, 1, 2) or self._chain_mode not in (0, 1):
            raise ValueError("persist_mode must be 0, 1 or 2 and chain_mode 0 or 1")
        self._tail_stream = bool(tail_stream)
        self._cond_stream = bool(cond_stream)
        self._gate_hs_stream = bool(gate_hs_stream)
        self._packed = None
        self._ws = {}
        self._wws = {}              # windowed synthesis: workspaces of several shapes side by side (_window_workspace)
        self._lib = _lib.load()    # fails loudly when libfwn.so is missing
        self.hop = int(np.prod(hparams.upsample_scales))
        if self.hop != hparams.hop_size:
            raise ValueError("prod(upsample_scales)=%d must equal hop_size=%d (model.py:231)"
                             % (self.hop, hparams.hop_size))

    # ------------------------------------------------------------------ parameters
    def load_params(self, params):
        """params: dict name -> array in the reference's layouts (weights.param_shapes)."""
        shapes = weights.param_shapes(self._hparams)
        for name, shape in shapes.items():
            if name not in params:
                raise KeyError("missing parameter %r" % name)
            got = tuple(getattr(params[name], "shape", None) or np.shape(params[name]))
            if got != tuple(shape):
                raise ValueError("parameter %r has shape %r, expected %r" % (name, got, tuple(shape)))
        self._packed = packing.pack_model(params, self._hparams, self._device, self._cond_mode, gate_fp8=self._gate_fp8,
                                          persist_mode=self._persist_mode, chain_mode=self._chain_mode, tail_stream=self._tail_stream,
                                          cond_stream=self._cond_stream, gate_hs_stream=self._gate_hs_stream)
        return self

    def init_synthetic(self, seed=1234, **kw):
        return self.load_params(weights.synthetic_params(self._hparams, seed, **kw))

    def export_actnorm(self):
        """ActNorm (b, logs) per flow in the reference's layout (after a DDI forward)."""
        out = {}
        hp = self._hparams
        for i in range(hp.n_block):
            for j in range(hp.n_flow):
                an = self._packed.an[(i, j)].cpu().numpy()
                b, logs = packing.actnorm_from_table(an, i)
                out[weights.flow_prefix(i, j) + "/ActNorm/b"] = b
                out[weights.flow_prefix(i, j) + "/ActNorm/logs"] = logs
        return out

    @property
    def weight_bytes(self):
        return self._packed.weight_bytes

    # ------------------------------------------------------------------ helpers
    def _check_g(self, g):
        if g is None and self._hparams.gin_channels > 0:
            raise ValueError("g is None")   # model.py:320-321,353-354

    def _require_params(self):
        if self._packed is None:
            raise RuntimeError("no parameters loaded: call load_params() / init_synthetic() first")

    def _check_c(self, c):
        if c.dim() != 3 or c.shape[2] != self._hparams.num_mels:
            raise ValueError("c must have shape [B, T/hop, %d], got %r" % (self._hparams.num_mels, tuple(c.shape)))

    def _prep(self, x, c, what):
        import torch
        self._require_params()
        hp = self._hparams
        if x.dim() != 3 or x.shape[2] != 1:
            raise ValueError("%s must have shape [B, T, 1], got %r" % (what, tuple(x.shape)))
        self._check_c(c)
        b, t = int(x.shape[0]), int(x.shape[1])
        if c.shape[0] != b or int(c.shape[1]) * self.hop != t:
            raise ValueError("c has %d frames for T=%d samples (hop_size=%d)" % (c.shape[1], t, self.hop))
        if t % (1 << hp.n_block):
            raise ValueError("T=%d must be a multiple of 2^n_block=%d (model.py:226)" % (t, 1 << hp.n_block))
        dev = torch.device(self._device)
        x32 = x.to(device=dev, dtype=torch.float32).contiguous()
        c32 = c.to(device=dev, dtype=torch.float32).contiguous()
        return b, t, x32, c32

    def _workspace(self, b, t, ragged=False):
        """Scratch for one pass.  One workspace per (B, T, HIP stream): passes issued on different
        streams (e.g. a forward and an inverse overlapping on the chip) never share scratch.  A ragged inverse
        (``reverse(..., lengths=)``) keeps a workspace of its own: it also holds the masked copy of the mel.  So does a
        ragged forward (``ragged="forward"``): one flow's ZeroConv output and the per-clip log-det sums on top of that; and a
        ragged init (``ragged="init"``): the chunk sums of the masked moments on top of those."""
        name = {"forward": "fwn_ragged_forward_workspace_bytes", "init": "fwn_ragged_init_workspace_bytes"}.get(
            ragged, "fwn_ragged_workspace_bytes") if ragged else "fwn_workspace_bytes"
        return self._cached_workspace(self._ws, self._ws_key(b, t, ragged), name, (b, t), lambda: self._keep_shape(b, t))

    def _cached_workspace(self, cache, key, name, args, evict):
        """``cache[key]`` as (256-byte aligned pointer, bytes from there).  A missing entry is allocated: ``lib.<name>(model,
        *args)`` bytes (0 is the library's refusal of the shape) and 256 to align in, after ``evict()`` has made room in the cache."""
        import torch
        ws = cache.get(key)
        if ws is None:
            n = getattr(self._lib, name)(C.byref(self._packed.model_desc), *args)
            if n == 0:
                _lib.check(-1, name)
            evict()
            ws = cache[key] = torch.empty(n + 256, dtype=torch.uint8, device=self._device)
        off = (-ws.data_ptr()) % 256
        return ws.data_ptr() + off, ws.numel() - off

    def _keep_shape(self, b, t):
        for k in [k for k in self._ws if k[:2] != (b, t)]:
            del self._ws[k]   # keep only the current shape's workspaces

    def _ws_key(self, b, t, ragged=False):
        return (b, t, self._stream()) + ((("ragged", ragged) if ragged in ("forward", "init") else ("ragged",)) if ragged else ())

    def _stream(self):
        import torch
        return torch.cuda.current_stream(torch.device(self._device)).cuda_stream

    def persist_status(self, b, t):
        """0 unless a one-launch flow (csrc/flow_persist.h) of the last ``forward`` / ``reverse`` with batch ``b`` and length ``t`` on
        the current stream gave up a bounded dependency wait (a pass that was only delayed - a preempted queue, a debugger -
        can: its log_p / logdet / waveform are NaN then).  > 0: the give-up code; retry, or build the model with
        ``persist_mode=1``.  0 as well where no pass of that shape has run on this stream yet (its workspace holds nothing to
        read).  Synchronises the stream (``fwn_model_persist_status``)."""
        if (b, t, self._stream()) not in self._ws:
            return 0
        ws, _ = self._workspace(b, t)
        return int(self._lib.fwn_model_persist_status(C.byref(self._packed.model_desc), b, t, ws, self._stream()))

    # ------------------------------------------------------------------ reference surface
    def forward(self, x, c, g=None, return_z=False, lengths=None):
        """x [B,T,1], c [B,T/hop,num_mels] -> (log_p, logdet) fp32 0-dim tensors (model.py:317-347).

        lengths (a list, NumPy array or tensor of B sample counts, the rules of ``reverse``): a ragged batch.  ``log_p`` and
        ``logdet`` are then fp32 tensors of shape [B]: entry ``b`` is what ``forward(x[b:b+1, :lengths[b]], c[b:b+1,
        :lengths[b] // hop])`` returns for that clip alone (to rounding) - the prior mean over the clip's own samples, the
        coupling means over its own rows.  Whatever (finite) ``x`` and ``c`` hold past a clip's length reaches no output
        bit; with ``return_z`` the planes are exactly 0 there, and ``reverse(z, c, lengths=lengths)`` inverts them.
        ``init=True`` (the data-dependent init of a ragged batch is ``forward_init``) and ``gate_fp8`` models raise ``ValueError``."""
        import torch
        self._check_g(g)
        b, t, x32, c32 = self._prep(x, c, "x")
        if lengths is not None:
            return self._forward_ragged(b, t, x32, c32, return_z, lengths)
        wsp, wsn = self._workspace(b, t)
        out2 = torch.empty(2, dtype=torch.float32, device=self._device)
        zp = torch.empty(2, b, t // 2, dtype=torch.float32, device=self._device) if return_z else None
        if self._init and self._dp_world() > 1:
            self._forward_init_dp(b, t, x32, c32, wsp, wsn, out2, zp)
        else:
            rc = self._lib.fwn_model_forward(C.byref(self._packed.model_desc), b, t, x32.data_ptr(), c32.data_ptr(),
                                             wsp, wsn, out2.data_ptr(), zp.data_ptr() if return_z else None,
                                             1 if self._init else 0, self._stream())
            _lib.check(rc, "fwn_model_forward")
        self._init = False       # the reference feeds init=True for one step only (train.py:221,229)
        if return_z:
            return out2[0], out2[1], zp
        return out2[0], out2[1]

    def _forward_ragged(self, b, t, x32, c32, return_z, lengths):
        import torch
        if self._init:
            raise ValueError("init=True takes no lengths: the data-dependent ActNorm init of a ragged batch is forward_init(x, c, lengths)")
        lens = self._device_lengths(lengths, b, t)
        wsp, wsn = self._workspace(b, t, ragged="forward")
        out = torch.empty(2, b, dtype=torch.float32, device=self._device)
        zp = torch.empty(2, b, t // 2, dtype=torch.float32, device=self._device) if return_z else None
        rc = self._lib.fwn_model_forward_ragged(C.byref(self._packed.model_desc), b, t, x32.data_ptr(), c32.data_ptr(),
                                                lens.data_ptr(), wsp, wsn, out.data_ptr(), zp.data_ptr() if return_z else None,
                                                self._stream())
        _lib.check(rc, "fwn_model_forward_ragged")
        return (out[0], out[1], zp) if return_z else (out[0], out[1])

    def forward_init(self, x, c, lengths, g=None, return_z=False):
        """The ActNorm data-dependent init from a ragged batch, whatever ``init=`` the constructor got: flow by flow, ``b`` and
        ``logs`` from the per-channel mean and mean square over the union of the clips' own rows - nothing past a clip's length
        is read or counted - and then the flow as ``forward(..., lengths=)`` runs it.  The tables stay in the packed model
        (``export_actnorm()``), and the next ``forward`` is a plain one.  -> per-clip ``(log_p [B], logdet [B])`` (and the
        planes [2][B][T/2], exactly 0 past each clip, with ``return_z``).  ``lengths``: the rules of ``forward``.  In a
        data-parallel job (``group``) the moments AND the row count are all-reduced flow by flow, so ranks holding different
        amounts of audio are weighted by it and every rank derives the same tables.  ``gate_fp8`` models raise ``ValueError``."""
        import torch
        self._check_g(g)
        b, t, x32, c32 = self._prep(x, c, "x")
        lens = self._device_lengths(lengths, b, t)
        wsp, wsn = self._workspace(b, t, ragged="init")
        out = torch.empty(2, b, dtype=torch.float32, device=self._device)
        zp = torch.empty(2, b, t // 2, dtype=torch.float32, device=self._device) if return_z else None
        cb, failure = None, []
        if self._dp_world() > 1:
            cb = self._reduce_callback(self._ws[self._ws_key(b, t, "init")], failure)
        rc = self._lib.fwn_model_forward_init_ragged(C.byref(self._packed.model_desc), b, t, x32.data_ptr(), c32.data_ptr(),
                                                     lens.data_ptr(), wsp, wsn, out.data_ptr(), zp.data_ptr() if return_z else None,
                                                     cb, None, self._stream())
        if failure:
            raise failure[0]
        _lib.check(rc, "fwn_model_forward_init_ragged")
        self._init = False
        return (out[0], out[1], zp) if return_z else (out[0], out[1])

    def _dp_world(self):
        import torch.distributed as dist
        if self._group is False or not (dist.is_available() and dist.is_initialized()):
            return 1                    # group=False: this model lives on one rank only (its init uses the local batch)
        return dist.get_world_size(self._group)

    def _forward_init_dp(self, b, t, x32, c32, wsp, wsn, out2, zp):
        """init=True on one rank of a data-parallel job: ``fwn_model_forward_init`` calls back before each flow's
        ActNorm tables are derived; the callback all-reduces that flow's 4 Ch + 1 moment doubles (RCCL; they live
        inside this pass's workspace tensor) in stream order."""
        failure = []
        cb = self._reduce_callback(self._ws[(b, t, self._stream())], failure)
        rc = self._lib.fwn_model_forward_init(C.byref(self._packed.model_desc), b, t, x32.data_ptr(), c32.data_ptr(),
                                              wsp, wsn, out2.data_ptr(), zp.data_ptr() if zp is not None else None,
                                              cb, None, self._stream())
        if failure:
            raise failure[0]
        _lib.check(rc, "fwn_model_forward_init")

    def _reduce_callback(self, ws, failure):
        """The ``fwn_reduce_fn`` of a data-parallel init pass running in the workspace tensor ``ws``: an in-place all-reduce of
        the n doubles at ``buf`` (inside ``ws``) in stream order; what it raises lands in ``failure``."""
        import torch
        from . import distributed
        base = ws.data_ptr()

        def reduce(user, buf, n, stream):
            try:
                off = int(buf) - base
                distributed.allreduce_sum_(ws[off:off + 8 * n].view(torch.float64), self._group)
                return 0
            except BaseException as e:      # must not propagate through the C frame
                failure.append(e)
                return 1

        return _lib.REDUCE_FN(reduce)

    def _check_lengths(self, lengths, b, t):
        """``lengths`` of a ragged ``reverse`` / ``forward`` -> list of B ints, validated on the host before anything is launched."""
        return check_lengths(lengths, b, t, self.hop, self._hparams.n_block)

    def _device_lengths(self, lengths, b, t, fp8_ok=False):
        """``lengths`` -> the int32 device tensor a ragged pass reads; a ``gate_fp8`` model has no such pass."""
        import torch
        if self._gate_fp8 and not fp8_ok:
            raise ValueError("a gate_fp8 model takes no lengths: the e4m3 copies of h are not masked")
        return torch.tensor(self._check_lengths(lengths, b, t), dtype=torch.int32).to(self._device)

    def reverse(self, z, c, g=None, dtype=None, lengths=None):
        """z [B,T,1], c [B,T/hop,num_mels] -> x [B,T,1] (model.py:350-396).  fp32 unless ``dtype`` is given: a torch dtype, or
        "hparams" for the reference's return type, ``hparams.dtype`` (float16 / bfloat16 / float32; model.py:356-357,396).

        lengths (a list, NumPy array or tensor of B sample counts): a ragged batch.  Clip ``b`` is ``z[b, :lengths[b]]``
        with ``c[b, :lengths[b] // hop]``; ``x[b, :lengths[b]]`` is what ``reverse`` gives for that clip alone (to
        rounding) and ``x[b, lengths[b]:]`` is 0.  Whatever (finite) ``z`` and ``c`` hold past a clip's length reaches no
        output bit.  Every length must be a multiple of lcm(hop_size, 2^n_block), at least that, at most T
        (``ValueError`` otherwise).  ``gate_fp8`` models do not take lengths.  None: the plain pass."""
        import torch
        self._check_g(g)
        if dtype == "hparams":
            dtype = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}[str(self._hparams.dtype).replace("tf.", "")]
        b, t, z32, c32 = self._prep(z, c, "z")
        lens = None if lengths is None else self._device_lengths(lengths, b, t)
        wsp, wsn = self._workspace(b, t, ragged=lengths is not None)
        x = torch.empty(b, t, 1, dtype=torch.float32, device=self._device)
        if lengths is None:
            rc = self._lib.fwn_model_reverse(C.byref(self._packed.model_desc), b, t, z32.data_ptr(), c32.data_ptr(),
                                             wsp, wsn, x.data_ptr(), self._stream())
            _lib.check(rc, "fwn_model_reverse")
        else:
            rc = self._lib.fwn_model_reverse_ragged(C.byref(self._packed.model_desc), b, t, z32.data_ptr(), c32.data_ptr(),
                                                    lens.data_ptr(), wsp, wsn, x.data_ptr(), self._stream())
            _lib.check(rc, "fwn_model_reverse_ragged")
        return x if dtype is None or dtype == torch.float32 else x.to(dtype)

    # ------------------------------------------------------------------ device-side synthesis
    def _clip_ids(self, clip_ids, b):
        """``clip_ids`` -> device tensor holding B uint32 (as int32 bits), or None: clip b is b."""
        import torch
        if clip_ids is None:
            return None
        return torch.from_numpy(np.asarray(self._clip_id_values(clip_ids, b), dtype=np.uint32).view(np.int32)).to(self._device)

    @staticmethod
    def _clip_id_values(clip_ids, b):
        """``clip_ids`` -> list of B ints in [0, 2^32), validated on the host."""
        vals = clip_ids.detach().cpu().tolist() if hasattr(clip_ids, "detach") else np.asarray(clip_ids).tolist()
        if not isinstance(vals, list) or len(vals) != b:
            raise ValueError("clip_ids must hold one id per clip (B=%d), got %r" % (b, vals))
        for v in vals:
            if int(v) != v or not 0 <= v < (1 << 32):
                raise ValueError("clip ids are integers in [0, 2^32), got %r" % (v,))
        return [int(v) for v in vals]

    def sample_z(self, b, t, seed, clip_ids=None, lengths=None, temp=None):
        """The latent of ``b`` clips of ``t`` samples, drawn on the device: fp32 [b, t, 1] = temp * N(0,1) (``temp``: default
        ``hparams.temp``) from a Philox4x32-10 stream keyed by (``seed`` mod 2^64, clip id) - include/fwn.h
        ``fwn_latent_normal``.  ``clip_ids`` (B integers in [0, 2^32); None: 0 .. b-1) name the clips: sample i of a clip
        depends on (seed, clip id, i, temp) only, so a clip draws the same z whichever batch, row or T it is given.
        ``lengths`` (the rules of ``reverse``): z is +0 from each clip's length on, and unchanged before it."""
        import torch
        b, t = int(b), int(t)
        if b < 1 or t < 1:
            raise ValueError("b and t must be positive, got %d, %d" % (b, t))
        ids = self._clip_ids(clip_ids, b)
        lens = None if lengths is None else self._device_lengths(lengths, b, t, fp8_ok=True)
        z = torch.empty(b, t, 1, dtype=torch.float32, device=self._device)
        rc = self._lib.fwn_latent_normal(z.data_ptr(), b, t, int(seed) % (1 << 64), None if ids is None else ids.data_ptr(),
                                         float(self._hparams.temp if temp is None else temp),
                                         None if lens is None else lens.data_ptr(), self._stream())
        _lib.check(rc, "fwn_latent_normal")
        return z

    def synthesize(self, c, seed, clip_ids=None, lengths=None, temp=None, return_wav=False, return_z=False):
        """c [B,F,num_mels] -> 16-bit PCM, ``torch.int16`` [B, F*hop] on the device, in one call: the latent of ``sample_z(B,
        F*hop, seed, clip_ids, lengths, temp)``, ``reverse`` (with ``lengths``: the ragged pass, same rules and refusals), and
        ``rint(clip(x, -1, 1) * 32767)`` in float64 with halves to even (NaN -> 0) - the arithmetic of
        ``synthesize.write_wav``.  Nothing touches the host.  Past a clip's length the PCM, the waveform and z are 0.
        return_wav / return_z add the fp32 waveform [B,T,1] / the latent [B,T,1] to the result, in that order."""
        import torch
        self._require_params()
        hp = self._hparams
        self._check_c(c)
        b, t = int(c.shape[0]), int(c.shape[1]) * self.hop
        if b < 1 or t < 1 or t % (1 << hp.n_block):
            raise ValueError("T=%d must be a positive multiple of 2^n_block=%d (model.py:226)" % (t, 1 << hp.n_block))
        c32 = c.to(device=torch.device(self._device), dtype=torch.float32).contiguous()
        ids = self._clip_ids(clip_ids, b)
        lens = None if lengths is None else self._device_lengths(lengths, b, t)
        wsp, wsn = self._synth_workspace(b, t, lens is not None)
        pcm = torch.empty(b, t, dtype=torch.int16, device=self._device)
        wav = torch.empty(b, t, 1, dtype=torch.float32, device=self._device) if return_wav else None
        z = torch.empty(b, t, 1, dtype=torch.float32, device=self._device) if return_z else None
        rc = self._lib.fwn_model_synthesize(C.byref(self._packed.model_desc), b, t, c32.data_ptr(), int(seed) % (1 << 64),
                                            None if ids is None else ids.data_ptr(), float(hp.temp if temp is None else temp),
                                            None if lens is None else lens.data_ptr(), wsp, wsn, pcm.data_ptr(),
                                            wav.data_ptr() if return_wav else None, z.data_ptr() if return_z else None,
                                            self._stream())
        _lib.check(rc, "fwn_model_synthesize")
        return pcm if not (return_wav or return_z) else (pcm,) + ((wav,) if return_wav else ()) + ((z,) if return_z else ())

    def _synth_workspace(self, b, t, ragged):
        """``_workspace`` for ``synthesize``: the inverse pass's scratch with z and the fp32 waveform behind it."""
        return self._cached_workspace(self._ws, (b, t, self._stream(), "synth", bool(ragged)), "fwn_synthesize_workspace_bytes",
                                      (b, t, 1 if ragged else 0), lambda: self._keep_shape(b, t))

    # ------------------------------------------------------------------ windowed passes (windowed.py drives them)
    def _window_workspace(self, kind, n, length):
        """Scratch of one group of ``n`` windows of ``length`` samples (``kind``: "reverse" - the plain inverse pass's -,
        "synth" - with z, the waveform and the windows' mel rows behind it - or "forward" - the windowed forward pass's, with
        every tail's ZeroConv output, the per-window sums and the windows' audio and mel rows).  A cache of its own, keyed by shape and stream: a
        long clip alternates between a few shapes (first, middle, end windows) and ``_workspace`` keeps one shape only.  The
        eight most recently used are kept; a size depends on (n, length) alone, never on a clip's length."""
        key = (kind, n, length, self._stream())
        if key in self._wws:
            self._wws[key] = self._wws.pop(key)      # re-inserted last: the dict's order is the order of use
        name = {"synth": "fwn_synthesize_windows_workspace_bytes", "forward": "fwn_forward_windows_workspace_bytes"}.get(
            kind, "fwn_workspace_bytes")

        def evict():
            while len(self._wws) >= 8:
                del self._wws[next(iter(self._wws))]
        return self._cached_workspace(self._wws, key, name, (n, length), evict)

    # the device calls of a group of windows, methods of the model: what a stand-in model under a stream replaces
    _windows_call = windowed.synthesize_windows_call
    _forward_windows_call = windowed.forward_windows_call
    _forward_windows_finish = windowed.forward_windows_finish

    def reverse_windowed(self, z, c, window, batch=8, halo=None, g=None):
        """``reverse(z, c)`` of clips of any length, window by window: z [B,T,1], c [B,T/hop,num_mels] -> x [B,T,1] fp32, T a
        multiple of lcm(hop_size, 2^n_block).  ``windowing.plan_windows(T, window, hparams, halo)`` cuts every clip into cores
        of ``window`` samples with ``windowing.halo_samples`` of real context on both sides; windows of equal length - of all
        clips - share a plain rectangular inverse pass, ``batch`` at a time, and each core is copied into the result.  With the
        default halo the result is the whole-clip pass's to rounding (exactly, in exact arithmetic: the halo covers the
        network's receptive field), and T is bounded by memory for z, c and x only, not by what one pass can address.
        ``halo`` (a multiple of the unit; 0 = hard cuts) is for experiments.  Host sequencing only: slices, the inverse pass,
        copies."""
        return windowed.reverse_windowed(self, z, c, window, batch, halo, g)

    def synthesize_windowed(self, c, seed, clip_ids=None, window=None, batch=8, temp=None, return_wav=False, halo=None):
        """``synthesize`` for clips of any length: c [B,F,num_mels] -> 16-bit PCM, ``torch.int16`` [B, F*hop] on the device, F*hop
        a multiple of lcm(hop_size, 2^n_block).  The clips are cut by ``windowing.plan_windows(F*hop, window, hparams, halo)``
        (``window`` in samples; default 65 536 rounded up to the unit); windows of equal length, of all clips, share a call,
        ``batch`` at a time, and each call is ``fwn_model_synthesize_windows``: the window's slice of the clip's latent stream,
        its mel rows gathered from ``c``, the plain inverse pass, the cores written into the result as PCM - all on the device.
        z is exactly ``sample_z``'s stream of (seed, clip id) (``clip_ids``: None = 0 .. B-1), so a clip's latent depends on
        neither ``window`` nor ``batch``; the waveform is the whole-clip pass's to rounding (``reverse_windowed``).  No ceiling
        on T other than memory for the mel and the PCM, and 2^34 samples per clip.  The scratch depends on (batch, window)
        alone.  ``return_wav`` adds the fp32 waveform [B,T,1]."""
        return windowed.synthesize_windowed(self, c, seed, clip_ids, window, batch, temp, return_wav, halo)

    def stream(self, seed, clip_id=0, window=None, temp=None, halo=None):
        """Synthesis of one clip whose mel arrives while it is being made: -> a ``SynthesisStream`` with ``push(frames)`` and
        ``finish()``.  Fed the frames of ``c`` in any split, the concatenated output is ``synthesize_windowed(c, seed, [clip_id],
        window, batch=1)`` bit for bit (the same windows, one call each); core k comes out of the push that delivers frame
        ``(b_k + H) / hop``."""
        self._require_params()
        return SynthesisStream(self, seed, clip_id, window, temp, halo)

    def forward_windowed(self, x, c, window=None, batch=8, return_z=False, halo=None, g=None):
        """``forward(x, c)`` of clips of any length, window by window: x [B,T,1], c [B,T/hop,num_mels] -> ``(log_p [B], logdet
        [B])`` fp32, entry b what ``forward`` gives for clip b alone (to rounding); T a multiple of lcm(hop_size, 2^n_block), at
        most 2^34.  The forward pass has the inverse pass's receptive field, so the clips are cut as for synthesis -
        ``windowing.plan_windows(T, window, hparams, halo)``, ``window`` in samples (default: ``synthesize_windowed``'s) - and
        windows of equal length, of all clips, share a ``fwn_model_forward_windows`` call, ``batch`` at a time: audio and mel
        rows gathered on the device, the rectangular pass, and the fp64 sums of z^2 and -log_s over each window's CORE only
        (a window's own scalars would include its halo).  One more launch adds every clip's windows in window order: the
        result depends on neither ``batch`` nor the order of the calls, and two identical calls give identical bits.
        ``return_z`` adds z [B,T,1] fp32 in TIME order - the latent ``reverse`` / ``reverse_windowed(z, c, window)`` take and
        invert.  No ceiling on T other than memory for x, c and z; the scratch depends on (batch, window) alone.  ``halo`` (0
        = hard cuts) is for experiments.  ``init=True`` and ``gate_fp8`` models raise ``ValueError``."""
        return windowed.forward_windowed(self, x, c, window, batch, return_z, halo, g)

    def forward_stream(self, window=None, halo=None, return_z=True):
        """The likelihood and the latent of one clip that is still arriving: -> a ``ForwardStream`` with ``push(x_samples,
        c_frames)`` and ``finish()``.  Fed the clip in any split, the concatenated z cores and the scalars are
        ``forward_windowed(x, c, window, batch=1, return_z=True)`` bit for bit (the same windows, one call each)."""
        windowed.check_forward(self)
        return ForwardStream(self, window, halo, return_z)

    def upsample(self, c):
        """c [B,F,num_mels] -> [B,F*hop,num_mels] fp32 (model.py:398-404)."""
        import torch
        if self._packed is None:
            raise RuntimeError("no parameters loaded")
        hp = self._hparams
        cur = c.to(device=self._device, dtype=torch.float32).contiguous()
        md = self._packed.model_desc
        for n, s in enumerate(hp.upsample_scales):
            b, h, w = cur.shape
            out = torch.empty(b, h * s, w, dtype=torch.float32, device=self._device)
            rc = self._lib.fwn_upsample_stage(cur.data_ptr(), b, h, w, md.up_w[n], md.up_bias[n], int(s),
                                              out.data_ptr(), None, self._stream())
            _lib.check(rc, "fwn_upsample_stage")
            cur = out
        return cur

    __call__ = forward


def check_lengths(lengths, b, t, hop, n_block):
    """The lengths of a ragged batch (``FloWaveNet.forward`` / ``reverse``, ``training.GradEngine``) -> list of B ints, validated
    on the host before anything is launched: one integer per clip, a multiple of lcm(hop, 2^n_block), at least that, at most t."""
    import math
    vals = lengths.detach().cpu().tolist() if hasattr(lengths, "detach") else np.asarray(lengths).tolist()
    if not isinstance(vals, list) or len(vals) != b:
        raise ValueError("lengths must hold one length per clip (B=%d), got %r" % (b, vals))
    unit = math.lcm(hop, 1 << n_block)
    for v in vals:
        if int(v) != v:
            raise ValueError("lengths must be integers (samples), got %r" % (v,))
        if not unit <= v <= t:
            raise ValueError("length %d outside [%d, T=%d]" % (v, unit, t))
        if v % unit:
            raise ValueError("length %d must be a multiple of lcm(hop_size=%d, 2^n_block=%d) = %d"
                             % (v, hop, 1 << n_block, unit))
    return [int(v) for v in vals]


def z_planes_to_squeezed(zp, n_block, n_flow=2):
    """planes[2][B][T/2] (device layout) -> the reference's final ``out`` [B, T/2^n, 2^n]
    (logical squeezed channel order after n_block*n_flow change_orders), for comparisons
    against the oracle."""
    import torch
    two, b, ht = zp.shape
    n = n_block
    ch = 1 << (n - 1)
    rows = ht // ch
    v = zp.reshape(2, b, rows, ch)                       # [q][b][t][tau']
    br = torch.as_tensor(packing.bitrev_table(n - 1).astype(np.int64), device=zp.device)
    out = torch.empty(b, rows, 2 * ch, dtype=zp.dtype, device=zp.device)
    swapped = (n_block * n_flow) & 1                     # odd number of swaps: halves exchanged
    for q in range(2):
        out[:, :, (q ^ swapped) * ch + br] = v[q]
    return out
