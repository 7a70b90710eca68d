"""Fused train-step engine over libsignaltrain_hip.so.

Owns (as torch tensors -- PyTorch is the allocator, nothing more) the flat fp32 parameter /
gradient / Adam-moment buffers laid out by `st_param_offsets` and the workspace the C library
carves.  One engine = one GPU = one process; data parallelism (dp.py) all-reduces `grads`.

Reference mapping: one `train_step` call == the body of train_loop's minibatch iteration,
signaltrain/train.py:112-151 (forward, calc_loss, backward, clip_grad_norm_, Adam.step).
"""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib

AE_LAYERS = ("fnn_enc", "fnn_enc2", "fnn_enc3", "fnn_enc4", "fnn_addknobs",
             "fnn_dec4", "fnn_dec3", "fnn_dec2", "fnn_dec")          # nn_proc.py:64-65
STFT_KEYS = ("mpaec.dft_analysis.conv_analysis_real.weight",
             "mpaec.dft_analysis.conv_analysis_imag.weight",
             "mpaec.dft_synthesis.conv_synthesis_real.weight",
             "mpaec.dft_synthesis.conv_synthesis_imag.weight")
COMPUTE_DTYPES = tuple(_lib.PREC)       # "f32", "bf16", "bf16_all", "f16", "f16_all", "f32x3"


def param_names():
    """state_dict() key order of the reference st_model."""
    keys = list(STFT_KEYS)
    for ae in ("aenc", "phs_aenc"):
        for n in AE_LAYERS:
            keys += [f"mpaec.{ae}.{n}.weight", f"mpaec.{ae}.{n}.bias"]
    return keys


def param_shapes(d):
    R = 64
    ae = [(R, d.T), (R // 2, R), (R // 4, R // 2), (R // 4, R // 4), (R // 4, R // 4 + d.K),
          (R // 4, R // 4), (R // 2, R // 4), (R, R // 2), (d.OT, R)]           # nn_proc.py:46-61
    shapes = [(d.N, 1, d.N)] * 4
    for _ in range(2):
        for (o, i) in ae:
            shapes += [(o, i), (o,)]
    return shapes


class ParamLayout:
    """Names, shapes and float offsets of the 40 tensors inside the flat buffers."""

    def __init__(self, d):
        self.names = param_names()
        self.shapes = param_shapes(d)
        self.offsets, self.total = _lib.param_offsets(d)
        self.n_stft = self.offsets[4]

    def views(self, flat):
        out = OrderedDict()
        for n, s, o in zip(self.names, self.shapes, self.offsets):
            out[n] = flat[o:o + int(np.prod(s))].view(*s)
        return out


class _OptimizerView:
    """What misc.save_checkpoint needs from an optimizer: state_dict() in torch.optim.Adam's layout (train.py:228)."""

    def __init__(self, engine):
        self.engine = engine

    def state_dict(self):
        return self.engine.optimizer_state_dict()


class RecordingCode:
    """What StepEngine.encode_long() leaves of a recording: the code tensor (opaque, layout in csrc/st_decode.h), the signal tensor it was built from (the
    overlap-add reads its residual), its length n, the window count, and the geometry and compute dtype it is valid for."""
    __slots__ = ("code", "signal", "n", "nwin", "geometry", "compute_dtype")

    def __init__(self, code, signal, n, nwin, geometry, compute_dtype):
        self.code, self.signal, self.n, self.nwin, self.geometry, self.compute_dtype = code, signal, int(n), int(nwin), tuple(geometry), compute_dtype


_warned_channels_unsupported = False


# ---------------------------------------------------------------- the argument rules of the whole-signal inference entries, each stated once
# Plain functions of tensors: they take the device, K and the window count as arguments and need neither an engine nor the library
# (tests/test_infer_args_host.py runs them on CPU tensors).  `what` is the entry's name in front of every message.
def _pcm(t):
    """The ST_PCM_* value of a recording tensor."""
    return _lib.PCM_S16 if t.dtype == torch.int16 else _lib.PCM_F32


def _recording(what, name, t, device, nonempty=False):
    """A recording argument as the library takes it: a 1-D float32 or int16 tensor on `device`, contiguous, and cloned if it starts off the boundary the
    kernels' quads of four samples need (pcm_align in st_api.hip: 8 bytes for int16, 16 for float32)."""
    if not (torch.is_tensor(t) and t.dim() == 1 and t.device == device and t.dtype in (torch.float32, torch.int16) and (t.numel() >= 1 or not nonempty)):
        raise ValueError(f"{what}: {name} must be a {'non-empty ' if nonempty else ''}1-D float32 or int16 tensor on {device}")
    t = t.contiguous()
    return t.clone() if t.data_ptr() % (8 if t.dtype == torch.int16 else 16) else t


def _recording_pair(what, signal, target, device, first="signal"):
    """Input and target of a fit or a score: two recordings (_recording) of equal length in ONE format -- where the dtypes differ the int16 one becomes
    float32 by the C rule, (float)((double)s / 32767.0), in a fresh (so aligned) tensor."""
    signal, target = _recording(what, first, signal, device), _recording(what, "target", target, device)
    if signal.numel() != target.numel():
        raise ValueError(f"{what}: {first} has {signal.numel()} samples, target {target.numel()}")
    if signal.dtype != target.dtype:
        signal, target = ((t.double() / 32767.0).float() if t.dtype == torch.int16 else t for t in (signal, target))
    return signal, target


def _per_window(nwin, n):
    return f": one row, or one per window ({nwin} windows for {n} samples)"


def _knob_rows(what, knobs, K, device, allowed, per):
    """(knobs as a contiguous float32 [rows, K] tensor on `device`, rows); (None, 1) for a model without knobs.  A row count outside `allowed` is refused,
    `per` ends the message."""
    if not K:
        return None, 1
    kn = torch.as_tensor(knobs).to(device=device, dtype=torch.float32).reshape(-1, K).contiguous()
    rows = int(kn.shape[0])
    if rows not in allowed:
        raise ValueError(f"{what}: knobs has {rows} rows{per}")
    return kn, rows


def _knob_settings(what, knobs, K, nwin, n, device, strict=False):
    """(S knob settings as a contiguous float32 [S, rows, K] tensor on `device`, rows 1 or nwin; whether ONE setting came as a 1-D [K]).  [S, K] becomes
    [S, 1, K], and so does every other shape that is not 3-D unless `strict`: then only [S, K] and [S, rows, K] pass."""
    kn = torch.as_tensor(knobs).to(device=device, dtype=torch.float32)
    single = kn.dim() == 1
    whole = kn.dim() == 3 and int(kn.shape[1]) in (1, nwin) and int(kn.shape[2]) == K
    if strict and not (whole or (kn.dim() == 2 and int(kn.shape[1]) == K)):
        raise ValueError(f"{what}: knobs must be [S, {K}] or [S, rows, {K}] with one row per setting, or one per window ({nwin} windows for {n} samples), "
                         f"not {tuple(kn.shape)}")
    if kn.dim() == 3 and not whole:
        raise ValueError(f"{what}: knobs [S, rows, K] has {int(kn.shape[1])} rows per setting" + _per_window(nwin, n))
    kn = (kn if whole else kn.reshape(-1, 1, K)).contiguous()
    if int(kn.shape[0]) < 1:
        raise ValueError(f"{what}: no knob setting")
    return kn, single


def _adam_state(state, like, device):
    """(m, v, first step) of a knob fit: zeros and 1, or clones of what a previous call returned, float32 in the shape of the knobs `like`."""
    if state is None:
        return torch.zeros_like(like), torch.zeros_like(like), 1
    m, v, first = state
    m, v = (t.to(device=device, dtype=torch.float32).reshape(like.shape).contiguous().clone() for t in (m, v))
    return m, v, int(first)


class PredictStream:
    """A predict session of a StepEngine (StepEngine.open_stream; st_predict_stream_* in include/signaltrain_hip.h): C channels fed block by block in
    lockstep.  push() enqueues and returns device tensors; nothing synchronises with the host.  The parameter-only head of the workspace is built at open and
    rebuilt by refresh() -- which push() calls by itself when the engine has taken a train step since; after any other change of engine.params call refresh()."""

    def __init__(self, engine, channels=1, batch=None):
        self.engine, self.channels = engine, int(channels)
        B = int(batch or engine.max_batch)
        if B < 1 or self.channels < 1:
            raise ValueError(f"open_stream: channels = {channels}, batch = {B}")
        self.dims = d = engine._infer_dims("open_stream", B)
        lib = engine.lib
        if not lib.st_predict_supported(C.byref(d)):
            raise RuntimeError(f"open_stream: st_predict_supported refuses this geometry (T={d.T}, OT={d.OT}): the wide autoencoder geometries have no "
                               "predict session; predict_channels falls back to forward() batch by batch")
        self.state = torch.empty(int(lib.st_predict_stream_state_bytes(C.byref(d), self.channels)), dtype=torch.uint8, device=engine.device)
        self.ws = torch.zeros(int(lib.st_predict_stream_ws_bytes(C.byref(d))), dtype=torch.uint8, device=engine.device)
        self.s = _lib.st_predict_stream()
        self._open(self.s)

    def _open(self, s):
        e = self.engine
        e._call("st_predict_stream_open", C.byref(self.dims), _lib.ptr(e.params), self.channels, C.byref(s), _lib.ptr(self.state), _lib.ptr(self.ws), e._stream())
        self._built_at = e.step_count

    def reopen(self):
        """st_predict_stream_open again on the same tensors: zero samples received and the head rebuilt from the engine's current parameters."""
        self._open(self.s)

    def refresh(self):
        """Rebuild the parameter-only head from the engine's current parameters; the session's samples and counters stay."""
        self._open(_lib.st_predict_stream())

    received = property(lambda self: int(self.s.received), doc="samples per channel pushed so far")
    emitted = property(lambda self: int(self.s.emitted), doc="samples per channel emitted so far")
    pending = property(lambda self: int(self.s.held), doc="samples per channel held for windows still incomplete")
    closed = property(lambda self: bool(self.s.closed))

    def reset(self):
        """Back to zero samples received (host only); same geometry, channels, workspace."""
        _lib.check(self.engine.lib.st_predict_stream_reset(C.byref(self.s)), "st_predict_stream_reset")

    def plan(self, m, final=False):
        """(first window, windows, samples emitted per channel, samples held afterwards) of a push of m samples now: st_predict_stream_plan."""
        out4 = (C.c_longlong * 4)()
        _lib.check(self.engine.lib.st_predict_stream_plan(C.byref(self.dims), self.s.received, int(m), int(bool(final)), out4), "st_predict_stream_plan")
        return tuple(int(v) for v in out4)

    def push(self, block, knobs, final=False, out=None):
        """block: [C, m] (or 1-D for C == 1) float32 / int16 tensor on the engine's device, m % 4 == 0 unless final; knobs: [K] / [1, K] (all channels) or
        [C, K]; out: a float32 device tensor [C, >= emitted] (1-D for a 1-D block) with 16-byte aligned rows to write into.  Returns the [C, emitted]
        (1-D for a 1-D block) float32 device tensor this push completes -- possibly empty.  No host sync."""
        e, d, Cn = self.engine, self.dims, self.channels
        if self.s.closed:
            raise RuntimeError("PredictStream.push: the session is closed (a final push came before): reset()")
        if not (torch.is_tensor(block) and block.device == e.device and block.dtype in (torch.float32, torch.int16) and block.dim() in (1, 2)):
            raise ValueError(f"PredictStream.push: block must be a [C, m] (or 1-D) float32 or int16 tensor on {e.device}")
        flat = block.dim() == 1
        if flat:
            block = block.reshape(1, -1)
        if block.shape[0] != Cn or (flat and Cn != 1):
            raise ValueError(f"PredictStream.push: block has {block.shape[0]} channels, the session {Cn}")
        m = int(block.shape[1])
        if not final and m % 4:
            raise ValueError(f"PredictStream.push: m = {m} of a non-final push must be a multiple of 4")
        align = 8 if block.dtype == torch.int16 else 16
        pitch = (m + 3) // 4 * 4 if Cn == 1 else int(block.stride(0))
        if m and (block.stride(1) != 1 or pitch < m or pitch % 4 or block.data_ptr() % align):      # a view the kernels cannot read as aligned quads: one copy
            pitch = (m + 3) // 4 * 4
            copy = torch.empty(Cn, pitch, dtype=block.dtype, device=e.device)
            copy[:, :m] = block
            block = copy
        _, _, emit, _ = self.plan(m, final)
        opitch = (emit + 3) // 4 * 4
        if out is None:
            res = torch.empty(Cn, opitch, dtype=torch.float32, device=e.device)
        else:
            res = out.reshape(1, -1) if out.dim() == 1 else out
            if not (out.dtype == torch.float32 and out.device == e.device and out.dim() == (1 if flat else 2) and res.shape[0] == Cn and res.shape[1] >= emit
                    and (res.stride(1) == 1 or res.shape[1] <= 1) and res.data_ptr() % 16 == 0 and (Cn == 1 or (res.stride(0) % 4 == 0 and res.stride(0) >= emit))):
                raise ValueError(f"PredictStream.push: out must be a float32 [C, >= {emit}] tensor on {e.device} with unit sample stride and 16-byte aligned rows")
            opitch = opitch if Cn == 1 else int(res.stride(0))
        kn, rows = _knob_rows("PredictStream.push", knobs, d.K, e.device, (1, Cn), f": one row, or one per channel ({Cn})")
        if e.step_count != self._built_at:
            self.refresh()
        e._call("st_predict_stream_push", C.byref(d), _lib.ptr(e.params), C.byref(self.s), _pcm(block),
                C.c_void_p(block.data_ptr()) if m else None, m, pitch, int(bool(final)), _lib.ptr(kn), rows,
                C.c_void_p(res.data_ptr()) if emit else None, opitch, _lib.ptr(self.state), _lib.ptr(self.ws), e._stream())
        res = res[:, :emit]
        return res.reshape(-1) if flat else res


def workspace_bytes_upto(lib, dims, max_batch):
    """Bytes of ONE workspace that serves every batch of 1 .. max_batch windows at every arithmetic level and clip scope: st_workspace_bytes_max (the exact
    st_workspace_bytes is a function of all three and is monotonic in none of them: INTEGRATION.md "Sizing the workspace")."""
    n = int(lib.st_workspace_bytes_max(C.byref(dims.with_batch(int(max_batch)))))
    if n <= 0:
        _lib.check(-1, "st_workspace_bytes_max")
    return n


class StepEngine:
    """Holds device state for one model replica and drives the HIP step."""

    def __init__(self, dims, device="cuda:0", max_batch=None, compute_dtype="f32", loss_scale=None, clip_all=None):
        """compute_dtype: "f32" (default, the parity path); "f32x3" = fp32-grade STFT GEMMs on the bf16 matrix pipe (operands as three
        bfloat16 planes, six partial products, fp32 accumulation; same tolerance as "f32"); "bf16" / "f16" = 16-bit operands with fp32
        accumulation in the STFT GEMMs (BASELINE configs[2], [3] / [4]); "bf16_all" / "f16_all" = also in the autoencoder layers.  Parameters, gradients,
        loss and Adam are fp32 in every mode.  loss_scale: static loss scale of the step (default: 1 except 2**12 for the f16
        modes -- Apex's amp.scale_loss, train.py:134-135); clip_all: L1 clip over all parameters instead of the STFT tensors
        (train.py:136, what the reference does with Apex on; default: only in the f16 modes)."""
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("signaltrain_amd.StepEngine needs a ROCm device (there is no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._arith_checked = set()
        self.set_arithmetic(compute_dtype, loss_scale, clip_all)
        self.dims = dims
        self.max_batch = int(max_batch or dims.B)
        self.layout = ParamLayout(dims)
        n = self.layout.total
        z = lambda: torch.zeros(n, dtype=torch.float32, device=self.device)
        self.params, self.grads, self.m, self.v = z(), z(), z(), z()
        dmax = dims.with_batch(self.max_batch)
        # set_arithmetic() may change the mode of a live engine and the workspace depends on it (fp32 autoencoder layers keep their activations: 294 MB at B = 256;
        # the 16-bit modes carry operand copies): size it for the LARGEST mode, whatever arithmetic level `dims` happens to carry
        # ... and for every batch up to max_batch: the size is NOT monotonic in the batch (the split-K slab counts of the weight-gradient / synthesis GEMMs are picked per
        # batch: at the default geometry 585 windows need 85.6 MB more than 586, 178 windows 70 MB more than 179 at shrink 1) and an engine sized for its largest batch
        # serves smaller ones (a last partial batch, predict_long's remainder, validation): st_workspace_bytes_max, tens of ms of host arithmetic once per engine.
        nbytes = max(workspace_bytes_upto(self.lib, dims, self.max_batch), int(self.lib.st_workspace_bytes(C.byref(dmax))))
        self.ws = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self.scalars = torch.zeros(8, dtype=torch.float32, device=self.device)
        self.eval_acc = torch.zeros(8, dtype=torch.float64, device=self.device)      # st_eval_step's accumulator (eval_step / eval_reset / eval_read)
        self.stage = None            # packed live analysis gradient rows (data parallel, allocated on first use)
        self.named = self.layout.views(self.params)
        self.named_grads = self.layout.views(self.grads)
        self.step_count = 0
        self.trainable = _lib.GROUP_ALL      # ST_GROUP_* mask of the parameter groups train_step updates (set_trainable / sync_trainable)
        self._group_lag = [0, 0, 0, 0]       # steps each group sat out frozen: group_steps = step_count - lag
        self.generation = 0          # bumped by every call that overwrites the saved-for-backward state in the workspace
        self.dp = None               # st_dp* of the library-owned RCCL communicator (dp.DataParallel attaches it)
        self._pending = None

    def set_arithmetic(self, compute_dtype, loss_scale=None, clip_all=None):
        if compute_dtype not in _lib.PREC:
            raise ValueError(f"compute_dtype must be one of {COMPUTE_DTYPES}")
        self.compute_dtype = compute_dtype
        half = compute_dtype.startswith("f16")
        self.loss_scale = float(loss_scale) if loss_scale is not None else (4096.0 if half else 1.0)
        self.clip_all = bool(half if clip_all is None else clip_all)

    # ---------------------------------------------------------------- parameters / optimizer state
    def load_state_dict(self, sd):
        for k, v in self.named.items():
            src = sd[k]
            src = torch.as_tensor(np.asarray(src)) if not torch.is_tensor(src) else src
            v.copy_(src.to(device=self.device, dtype=torch.float32).reshape(v.shape))

    def state_dict(self):
        return OrderedDict((k, v.detach().clone()) for k, v in self.named.items())

    def optimizer_view(self):
        return _OptimizerView(self)

    def optimizer_state_dict(self, lr=None):
        """Adam state in torch.optim.Adam.state_dict() layout (40 per-parameter entries keyed by index, views of the flat
        moment buffers copied to the host) -- what the reference writes into its checkpoints (misc.py:28)."""
        from . import misc
        m, v = self.layout.views(self.m.detach().cpu()), self.layout.views(self.v.detach().cpu())
        steps = [self.group_steps[g] for g, sl in enumerate(misc.GROUP_SLICES) for _ in range(sl.stop - sl.start)]      # each parameter's own group step; 0 = never stepped
        return misc.adam_state_dict(steps, self.lr if lr is None else lr,
                                    [t.clone() for t in m.values()], [t.clone() for t in v.values()])

    def load_optimizer_state_dict(self, osd):
        """Restore exp_avg / exp_avg_sq / step from a torch.optim.Adam state_dict (the reference's 'optimizer' checkpoint entry;
        the reference itself never reads it back, train.py:229).  Returns the restored learning rate, or None if `osd` is not
        in that layout (nothing is changed then)."""
        from . import misc
        flat = misc.flatten_optimizer_state(osd, self.layout.shapes)
        if flat is None:
            return None
        for buf, key in ((self.m, "exp_avg"), (self.v, "exp_avg_sq")):
            for view, src in zip(self.layout.views(buf).values(), flat[key]):
                view.copy_(torch.from_numpy(src).to(self.device).reshape(view.shape))
        self.step_count = int(flat["step"])
        self.group_steps = [int(flat["steps"][sl.start]) for sl in misc.GROUP_SLICES]
        self.lr = float(flat["lr"])
        return self.lr

    lr = 0.0        # last learning rate handed to train_step (recorded for optimizer_state_dict)

    # ---------------------------------------------------------------- frozen parameter groups
    GROUP_NAMES = ("analysis", "synthesis", "aenc", "phs_aenc")
    GROUP_MODULES = ("mpaec.dft_analysis.", "mpaec.dft_synthesis.", "mpaec.aenc.", "mpaec.phs_aenc.")

    @staticmethod
    def group_mask(mask_or_names):
        """An ST_GROUP_* mask from a mask or from an iterable of group names ("analysis", "synthesis", "aenc", "phs_aenc", "frontend" = the first two)."""
        if isinstance(mask_or_names, (int, np.integer)):
            mask = int(mask_or_names)
        else:
            names = [mask_or_names] if isinstance(mask_or_names, str) else list(mask_or_names)
            bad = [n for n in names if n not in _lib.GROUP_SETS]
            if bad:
                raise ValueError(f"unknown parameter group(s) {bad}: the groups are {sorted(_lib.GROUP_SETS)}")
            mask = 0
            for n in names:
                mask |= _lib.GROUP_SETS[n]
        if not 0 <= mask <= _lib.GROUP_ALL:
            raise ValueError(f"group mask {mask} is not a set of the four ST_GROUP_* bits")
        return mask

    @property
    def group_steps(self):
        """Adam step number of each group so far, in the order analysis, synthesis, aenc, phs_aenc (torch's per-parameter state['step']): step_count less
        the steps the group sat out frozen.  step_count counts train_step calls; assigning to it moves every group along."""
        return [max(int(self.step_count) - lag, 0) for lag in self._group_lag]

    @group_steps.setter
    def group_steps(self, steps):
        steps = [int(s) for s in steps]
        if len(steps) != 4 or min(steps) < 0 or max(steps) > int(self.step_count):
            raise ValueError(f"group_steps: four step numbers in 0..step_count ({self.step_count}) expected, got {steps}")
        self._group_lag = [int(self.step_count) - s for s in steps]

    def set_trainable(self, mask_or_names):
        """The groups train_step updates from now on (default: all four).  A frozen group's parameters and Adam moments are not written and its step
        number stands still (st_train_step_groups in include/signaltrain_hip.h)."""
        mask = self.group_mask(mask_or_names)
        if mask == 0:
            raise ValueError("set_trainable: nothing trainable -- at least one parameter group has to train")
        self.trainable = mask
        return mask

    def sync_trainable(self, model):
        """Take the mask from the requires_grad flags of `model` (an st_model, or anything whose named_parameters() carry its names): a group is trainable
        iff all its parameters require grad -- what nn_proc.freeze_layers / st_model.freeze() leave behind.  The groups freeze as a whole: a group with
        mixed flags raises ValueError naming its tensors, and so does a model with nothing trainable."""
        flags = {n: bool(p.requires_grad) for n, p in model.named_parameters()}
        mask = 0
        for g, prefix in enumerate(self.GROUP_MODULES):
            mine = {n: f for n, f in flags.items() if n.startswith(prefix)}
            if not mine:
                raise ValueError(f"sync_trainable: the model has no parameters under {prefix!r}")
            if all(mine.values()):
                mask |= 1 << g
            elif any(mine.values()):
                raise ValueError(f"sync_trainable: group {self.GROUP_NAMES[g]!r} is partly frozen (a group freezes as a whole): "
                                 f"frozen {sorted(n for n, f in mine.items() if not f)}, trainable {sorted(n for n, f in mine.items() if f)}")
        if mask == 0:
            raise ValueError("sync_trainable: every parameter of the model is frozen -- nothing to train")
        self.trainable = mask
        return mask

    def _refuse_frozen(self, what):
        """The captured step and the data-parallel step update every group with one step number: no form with frozen groups."""
        if self.trainable != _lib.GROUP_ALL or len(set(self.group_steps)) != 1:
            raise NotImplementedError(f"{what}: no form with frozen parameter groups or with groups whose Adam step numbers differ "
                                      f"(trainable mask {self.trainable}, group steps {self.group_steps}); train_step takes both")

    # ---------------------------------------------------------------- plumbing
    def _dims(self, B):
        """The geometry for a batch of B windows + this engine's arithmetic: precision, loss scale and clip scope travel in
        st_dims with every call (there is no process-wide switch)."""
        if B > self.max_batch:
            raise RuntimeError(f"batch {B} exceeds the engine's workspace (max_batch={self.max_batch})")
        d = self.dims.with_batch(B)
        d.prec, d.loss_scale, d.clip_all = _lib.PREC[self.compute_dtype], self.loss_scale, int(self.clip_all)
        if (B, self.compute_dtype) not in self._arith_checked:
            # no silent arithmetic switch: where this geometry / batch cannot take the requested level (st_effective_prec, e.g. an odd batch
            # on the wide autoencoder path) say so once per (batch, dtype) and keep it readable in effective_dtype(B)
            self._arith_checked.add((B, self.compute_dtype))
            eff = int(self.lib.st_effective_prec(C.byref(d)))
            if eff != d.prec:
                import warnings
                name = {v: k for k, v in _lib.PREC.items()}.get(eff, str(eff))
                warnings.warn(f"signaltrain_amd: compute_dtype={self.compute_dtype!r} with batch {B} at this geometry (T={d.T}, OT={d.OT}) runs the "
                              f"autoencoder layers in fp32 (effective arithmetic {name!r}): the wide autoencoder path needs an even batch for 16-bit "
                              f"Linear layers", RuntimeWarning, stacklevel=3)
        return d

    def effective_dtype(self, B=None):
        """The arithmetic a batch of B windows actually runs in (st_effective_prec): compute_dtype, except where the geometry cannot take it."""
        d = self.dims.with_batch(self.max_batch if B is None else B)
        d.prec, d.loss_scale, d.clip_all = _lib.PREC[self.compute_dtype], self.loss_scale, int(self.clip_all)
        eff = int(self.lib.st_effective_prec(C.byref(d)))
        return {v: k for k, v in _lib.PREC.items()}.get(eff, str(eff))

    def _stream(self):
        """The current stream OF THIS ENGINE'S DEVICE (not of whatever device happens to be current)."""
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, name, *args):
        """One C-ABI call with this engine's device current: the library launches on the device that is current at call time
        (it never calls hipSetDevice itself), so an engine on cuda:1 must not depend on the caller's current device."""
        with torch.cuda.device(self.device):
            _lib.check(getattr(self.lib, name)(*args), name)

    def _prep(self, x, knobs, y=None):
        f = lambda t: None if t is None else t.to(device=self.device, dtype=torch.float32).contiguous()
        x, knobs, y = f(x), f(knobs), f(y)
        d = self._dims(x.shape[0])
        assert x.shape == (d.B, d.L) and knobs.shape == (d.B, d.K), (x.shape, knobs.shape, d.as_dict())
        if y is not None:
            assert y.shape == (d.B, d.y), (y.shape, d.y)
        if d.K == 0:
            knobs = None      # a model WITHOUT knobs (nn_proc.py:92-93 concatenates an empty [B, 0] tensor): an empty tensor has no data pointer; the C ABI takes NULL for K == 0
        return d, x, knobs, y

    # ---------------------------------------------------------------- forward / backward / step
    def forward(self, x, knobs, save_for_backward=False):
        """st_model.forward (nn_proc.py:392): returns (y_hat[B,y], mag[B,T,F], mag_hat[B,OT,F])."""
        d, x, knobs, _ = self._prep(x, knobs)
        y_hat = torch.empty(d.B, d.y, dtype=torch.float32, device=self.device)
        mag = torch.empty(d.B, d.T, d.F, dtype=torch.float32, device=self.device)
        mag_hat = torch.empty(d.B, d.OT, d.F, dtype=torch.float32, device=self.device)
        self.generation += 1
        self._call("st_model_fwd", C.byref(d), _lib.ptr(self.params), _lib.ptr(x), _lib.ptr(knobs),
                   _lib.ptr(y_hat), _lib.ptr(mag), _lib.ptr(mag_hat), _lib.ptr(self.ws), 1 if save_for_backward else 0, self._stream())
        return y_hat, mag, mag_hat

    def knob_grad(self, x, knobs, g_y_hat, g_mag_hat=None, g_mag=None):
        """d / d knobs [B, K] for the upstream gradients of backward() (st_model_knob_grad; nn_proc.py:92-93 under autograd).  The exact, slow route:
        one forward + backward per window.  Overwrites the workspace's saved-for-backward state (call forward(save_for_backward=True) again before
        backward()); the parameter gradients of these passes go to a scratch buffer, self.grads is left alone."""
        d, x, knobs, _ = self._prep(x, knobs)
        if d.K == 0:
            return torch.empty(d.B, 0, dtype=torch.float32, device=self.device)
        d.loss_scale = 0.0
        f = lambda t: None if t is None else t.to(device=self.device, dtype=torch.float32).contiguous()
        g_y_hat, g_mag_hat, g_mag = f(g_y_hat), f(g_mag_hat), f(g_mag)
        if getattr(self, "_knob_scratch", None) is None:
            self._knob_scratch = torch.zeros_like(self.grads)
        out = torch.empty(d.B, d.K, dtype=torch.float32, device=self.device)
        self.generation += 1
        self._call("st_model_knob_grad", C.byref(d), _lib.ptr(self.params), _lib.ptr(self._knob_scratch), _lib.ptr(x), _lib.ptr(knobs),
                   _lib.ptr(g_y_hat), _lib.ptr(g_mag_hat), _lib.ptr(g_mag), _lib.ptr(self.ws), _lib.ptr(out), self._stream())
        return out

    def backward(self, x, knobs, g_y_hat, g_mag_hat=None, g_mag=None):
        """Autograd backward for arbitrary upstream gradients (after forward(save_for_backward=True))."""
        d, x, knobs, _ = self._prep(x, knobs)
        d.loss_scale = 0.0                 # the upstream gradient is whatever autograd hands over: no loss scale of ours in it
        f = lambda t: None if t is None else t.to(device=self.device, dtype=torch.float32).contiguous()
        g_y_hat, g_mag_hat, g_mag = f(g_y_hat), f(g_mag_hat), f(g_mag)
        self._call("st_model_bwd", C.byref(d), _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(x),
                   _lib.ptr(knobs), _lib.ptr(g_y_hat), _lib.ptr(g_mag_hat), _lib.ptr(g_mag), _lib.ptr(self.ws), self._stream())
        return self.grads

    def knob_grad_fused_supported(self, B):
        """Whether backward_with_knob_grad() runs a batch of B windows at this engine's arithmetic (st_knob_grad_fused_supported: host arithmetic only).
        False for a model without knobs and where a diagnostic switch routes the autoencoder backward to a kernel form without the per-group output."""
        return bool(self.lib.st_knob_grad_fused_supported(C.byref(self._dims(int(B)))))

    def backward_with_knob_grad(self, x, knobs, g_y_hat, g_mag_hat=None, g_mag=None):
        """backward() and, in the same pass, d / d knobs [B, K] (st_model_bwd_knobs): returns (self.grads, g_knobs).  After forward(save_for_backward=True),
        like backward(); self.grads receives exactly what backward() writes and the workspace still holds the batch's state afterwards (knob_grad(), the
        exact per-window route, leaves the last window's).  Raises where knob_grad_fused_supported(B) is False."""
        if self.dims.K == 0:               # no knobs, no knob gradient: the plain backward and an empty [B, 0] tensor, without a st_model_bwd_knobs call
            return self.backward(x, knobs, g_y_hat, g_mag_hat, g_mag), torch.empty(x.shape[0], 0, dtype=torch.float32, device=self.device)
        d, x, knobs, _ = self._prep(x, knobs)
        d.loss_scale = 0.0
        f = lambda t: None if t is None else t.to(device=self.device, dtype=torch.float32).contiguous()
        g_y_hat, g_mag_hat, g_mag = f(g_y_hat), f(g_mag_hat), f(g_mag)
        need = int(self.lib.st_model_bwd_knobs_ws_floats(C.byref(d)))
        if getattr(self, "_knob_groups", None) is None or self._knob_groups.numel() < need:
            self._knob_groups = torch.empty(need, dtype=torch.float32, device=self.device)      # per-group column sums of d a5; never cleared (written before read)
        out = torch.empty(d.B, d.K, dtype=torch.float32, device=self.device)
        self._call("st_model_bwd_knobs", C.byref(d), _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(x), _lib.ptr(knobs),
                   _lib.ptr(g_y_hat), _lib.ptr(g_mag_hat), _lib.ptr(g_mag), _lib.ptr(self.ws), _lib.ptr(self._knob_groups), _lib.ptr(out), self._stream())
        return self.grads, out

    def input_grad(self, x, g_y_hat):
        """d loss / d x of the whole model (right after backward() on the same batch): half the conv-transpose of the analysis output
        gradient (nn_proc.py:307 feeds x/2) plus the skip connection's share on the last y samples (nn_proc.py:340)."""
        d = self._dims(x.shape[0])
        scratch = torch.empty(self.lib.st_model_input_grad_ws_floats(C.byref(d)), dtype=torch.float32, device=self.device)
        gx = torch.empty(d.B, d.L, dtype=torch.float32, device=self.device)
        self._call("st_model_input_grad", C.byref(d), _lib.ptr(self.params), _lib.ptr(self.ws), _lib.ptr(scratch), _lib.ptr(gx), self._stream())
        gx.mul_(0.5)
        if g_y_hat is not None:
            gx[:, d.L - d.y:] += g_y_hat.to(device=self.device, dtype=torch.float32)
        return gx

    def loss_backward(self, x, knobs, y, want_outputs=False):
        """forward + calc_loss (loss_functions.py:26-36 with scale_by_freq) + backward; fills self.grads (times the loss
        scale, if one is set).  self.scalars[0..4] = loss, mean log-cosh, L1 term, L1 norm of the (unscaled) STFT grads, clip coefficient."""
        d, x, knobs, y = self._prep(x, knobs, y)
        self._pending = (d, x, knobs, y)   # the dims clip_adam() carves the workspace with are those of the LAST backward
        outs = (None, None, None)
        if want_outputs:
            outs = (torch.empty(d.B, d.y, dtype=torch.float32, device=self.device),
                    torch.empty(d.B, d.T, d.F, dtype=torch.float32, device=self.device),
                    torch.empty(d.B, d.OT, d.F, dtype=torch.float32, device=self.device))
        self.generation += 1
        self._call("st_loss_backward", C.byref(d), _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(x),
                   _lib.ptr(knobs), _lib.ptr(y), _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]), _lib.ptr(self.ws),
                   _lib.ptr(self.scalars), self._stream())
        return outs

    def _stage_buf(self):
        if self.stage is None:
            self.stage = torch.zeros(2 * self.dims.F * self.dims.N, dtype=torch.float32, device=self.device)
        return self.stage

    def loss_backward_p1(self, x, knobs, y):
        """Forward + backward up to (excluding) the analysis weight gradient; see dp.DataParallel."""
        d, x, knobs, y = self._prep(x, knobs, y)
        self._pending = (d, x, knobs, y)
        self.generation += 1
        self._call("st_loss_backward_p1", C.byref(d), _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(x),
                   _lib.ptr(knobs), _lib.ptr(y), _lib.ptr(self.ws), self._stream())

    def loss_backward_p2(self):
        """Analysis weight gradient; the 2F live rows also land packed in self.stage (see grad_buckets)."""
        d, x = self._pending[:2]
        self._call("st_loss_backward_p2_staged", C.byref(d), _lib.ptr(self.grads), _lib.ptr(self._stage_buf()), _lib.ptr(x),
                   _lib.ptr(self.ws), _lib.ptr(self.scalars), self._stream())

    def finish_buckets(self):
        """After the all-reduce of grad_buckets(): copy the reduced analysis rows from the packed staging buffer back into grads."""
        self._call("st_unstage_analysis", C.byref(self._pending[0]), _lib.ptr(self.grads), _lib.ptr(self.stage), self._stream())

    N_STAGES = 4

    def loss_backward_stage(self, stage, x=None, knobs=None, y=None):
        """Stage `stage` (0..3, in order) of forward + loss + backward; stage 0 takes the minibatch.  After stage s the
        range stage_bucket(s) of self.grads is final (st_loss_backward_stage in include/signaltrain_hip.h)."""
        if stage == 0:
            self._pending = self._prep(x, knobs, y)
            self.generation += 1
        d, x, knobs, y = self._pending
        self._call("st_loss_backward_stage", C.byref(d), _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(x),
                   _lib.ptr(knobs), _lib.ptr(y), _lib.ptr(self.ws), _lib.ptr(self.scalars), int(stage), self._stream())

    def stage_bucket(self, stage):
        """Gradient range that is final after loss_backward_stage(stage): synthesis bases (4.2 MB at N=1024), both
        autoencoders (67 KB), live rows [0,F) of the real analysis basis, live rows of the imaginary one (2.1 MB each)."""
        o, d = self.layout.offsets, self.dims
        live = d.F * d.N
        return (self.grads[o[2]:o[4]], self.grads[o[4]:], self.grads[o[0]:o[0] + live], self.grads[o[1]:o[1] + live])[stage]

    def grad_buckets(self):
        """Two-phase form (loss_backward_p1 / _p2): the buffers to all-reduce, in the order they become final --
        [synthesis + autoencoders] = grads[offs[2]:] after phase 1, then the packed staging copy [2F][N] of the live analysis
        rows written by phase 2 (4.2 MB; the contiguous range of grads holding them would span 2 MB of structurally-zero rows).
        Call finish_buckets() after the second all-reduce."""
        return [self.grads[self.layout.offsets[2]:], self._stage_buf()]

    def train_step(self, x, knobs, y, lr, betas=(0.9, 0.999), eps=1e-8):
        """One optimisation step (train.py:112-151).  `lr` is the value sitting in param_groups at step
        time, i.e. lr_sched[max(i-1,0)] in the reference loop (train.py:150).  No host sync."""
        d, x, knobs, y = self._prep(x, knobs, y)
        self._pending = None               # a later clip_adam() must not carve the workspace with an older backward's dims
        if self.step_count == 0:
            self._group_lag = [0, 0, 0, 0]    # a reset optimizer (step_count = 0 with cleared moments): no group has a history
        self.step_count += 1; self.generation += 1; self.lr = float(lr)
        mask = int(self.trainable)
        self._group_lag = [lag if (mask >> g) & 1 else lag + 1 for g, lag in enumerate(self._group_lag)]      # a frozen group's step number stands still
        steps = self.group_steps
        if mask == _lib.GROUP_ALL and len(set(steps)) == 1:
            self._call("st_train_step", C.byref(d), _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self.m),
                       _lib.ptr(self.v), _lib.ptr(x), _lib.ptr(knobs), _lib.ptr(y), _lib.ptr(self.ws),
                       _lib.ptr(self.scalars), float(lr), float(betas[0]), float(betas[1]), float(eps),
                       int(steps[0]), self._stream())
        else:
            self._call("st_train_step_groups", C.byref(d), _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self.m),
                       _lib.ptr(self.v), _lib.ptr(x), _lib.ptr(knobs), _lib.ptr(y), _lib.ptr(self.ws),
                       _lib.ptr(self.scalars), float(lr), float(betas[0]), float(betas[1]), float(eps),
                       (C.c_int * 4)(*steps), mask, self._stream())
        return self.scalars

    # ---------------------------------------------------------------- validation on the device
    EVAL_FIELDS = ("vl_avg", "loss", "logcosh", "l1_term", "mae", "batches", "loss_sum", "mae_sum")

    def eval_step(self, x, knobs, y, beta=0.98, want_y_hat=False):
        """One validation batch (train.py:28-42) as one C call: the forward of train_step at this compute_dtype, calc_loss with scale_by_freq and mae,
        accumulated into self.eval_acc on the device (st_eval_step in include/signaltrain_hip.h).  No host sync; read with eval_read().  Overwrites the
        workspace's saved-for-backward state (a pending autograd backward recomputes its forward); parameters, gradients, moments and scalars are untouched."""
        d, x, knobs, y = self._prep(x, knobs, y)
        y_hat = torch.empty(d.B, d.y, dtype=torch.float32, device=self.device) if want_y_hat else None
        self.generation += 1
        self._call("st_eval_step", C.byref(d), _lib.ptr(self.params), _lib.ptr(x), _lib.ptr(knobs), _lib.ptr(y), _lib.ptr(y_hat),
                   _lib.ptr(self.ws), C.c_void_p(self.eval_acc.data_ptr()), float(beta), self._stream())
        return y_hat

    def eval_reset(self, vl_avg=0.0):
        """Start a validation pass: the running average is seeded with `vl_avg` (train.py carries it from epoch to epoch), everything else is zero."""
        self.eval_acc.zero_()
        self.eval_acc[0] = float(vl_avg)

    def eval_read(self):
        """The eight accumulator values (EVAL_FIELDS order) as Python floats: ONE device->host sync."""
        return self.eval_acc.tolist()

    # ---------------------------------------------------------------- whole-signal inference on the device
    def _infer_dims(self, what, batch):
        """The dims of an inference entry: `batch` rows per internal batch (default max_batch) at this engine's compute dtype, loss scale and clip scope."""
        B = int(batch or self.max_batch)
        if B < 1:
            raise ValueError(f"{what}: batch = {B}")
        d = self.dims.with_batch(B)
        d.prec, d.loss_scale, d.clip_all = _lib.PREC[self.compute_dtype], self.loss_scale, int(self.clip_all)
        return d

    def _kept(self, name):
        """A dict the inference entries keep on this engine from call to call (made on first use)."""
        return self.__dict__.setdefault(name, {})

    # an entry's own workspace, by attribute: (its size function, the gate behind a size of 0, where the wide autoencoder geometries stay)
    _OWN_WS = {"_predict_ws": ("st_predict_ws_bytes", "st_predict_supported", "forward()"),
               "_pool_ws": ("st_eval_pool_ws_bytes", "st_eval_pool_supported", "forward()"),
               "_decode_ws": ("st_decode_ws_bytes", "st_decode_supported", "predict_long's batched route"),
               "_fit_ws": ("st_fit_knobs_ws_bytes", "st_fit_knobs_supported", "the batched route"),
               "_multi_ws": ("st_knob_multi_ws_bytes", "st_fit_knobs_supported", "the batched route")}

    def _own_ws(self, what, attr, d, *more):
        """The workspace tensor self.<attr> an inference entry keeps for itself (_OWN_WS; `more`: what its size function takes behind the dims), allocated
        on first use and grown, never shrunk.  A size query carves every batch 1 .. B (milliseconds at B = 1024): asked once per (B, more, dtype)."""
        size_fn, gate, stay = self._OWN_WS[attr]
        sizes = self._kept("_own_ws_sizes")
        key = (attr, d.B, self.compute_dtype) + more
        if key not in sizes:
            sizes[key] = int(getattr(self.lib, size_fn)(C.byref(d), *more))
        if sizes[key] <= 0:
            raise RuntimeError(f"{what}: {gate} refuses this geometry (T={d.T}, OT={d.OT}): the wide autoencoder geometries stay on {stay}")
        ws = getattr(self, attr, None)
        if ws is None or ws.numel() < sizes[key]:
            ws = torch.zeros(sizes[key], dtype=torch.uint8, device=self.device)
            setattr(self, attr, ws)
        return ws

    def predict_supported(self):
        """Whether predict_long() runs this geometry (st_predict_supported: the fused autoencoder geometries; host arithmetic only)."""
        return bool(self.lib.st_predict_supported(C.byref(self.dims.with_batch(1))))

    def predict_long(self, signal, knobs, out=None, batch=None):
        """A whole recording through the model in ONE C call (st_predict_long in include/signaltrain_hip.h; utils/predict_long.py:30-79).
        signal: 1-D tensor on this engine's device, float32 or int16 (16-bit PCM, s / 32767); knobs: [K], [1, K] (one setting) or [nwin, K] (one row per
        window); batch: windows per internal batch (default max_batch); out: a float32 device tensor of at least n - (L - y) samples to write into.
        Returns the n - (L - y) predicted samples as a float32 device tensor (empty where the signal is shorter than the first window's lookback).  No host
        sync.  The engine keeps a workspace of its own for this (st_predict_ws_bytes, allocated on first use): self.ws is not written; generation moves on."""
        signal = _recording("predict_long", "signal", signal, self.device)
        d = self._infer_dims("predict_long", batch)
        n = int(signal.numel())
        nwin, n_out = int(self.lib.st_predict_windows(C.byref(d), n)), int(self.lib.st_predict_out_samples(C.byref(d), n))
        kn, rows = _knob_rows("predict_long", knobs, d.K, self.device, (1, nwin), _per_window(nwin, n))
        if out is None:
            out = torch.empty(n_out, dtype=torch.float32, device=self.device)
        elif not (out.dtype == torch.float32 and out.device == self.device and out.dim() == 1 and out.is_contiguous() and out.numel() >= n_out and out.data_ptr() % 16 == 0):
            raise ValueError(f"predict_long: out must be a contiguous, 16-byte aligned 1-D float32 tensor of at least {n_out} samples on {self.device}")
        ws = self._own_ws("predict_long", "_predict_ws", d)
        self.generation += 1
        if n_out > 0:
            self._call("st_predict_long", C.byref(d), _lib.ptr(self.params), _pcm(signal), C.c_void_p(signal.data_ptr()), n, _lib.ptr(kn), rows,
                       C.c_void_p(out.data_ptr()), _lib.ptr(ws), self._stream())
        return out[:n_out]

    # ---------------------------------------------------------------- a folder of recordings in one call
    def eval_pool_supported(self):
        """Whether eval_pool() runs this geometry (st_eval_pool_supported = st_predict_supported; host arithmetic only)."""
        return bool(self.lib.st_eval_pool_supported(C.byref(self.dims.with_batch(1))))

    def eval_pool(self, pool_x, pool_y, off, length, knobs, want_out=False, batch=None):
        """Every file of a device feed's pool WHOLE through the model, each at its own knob row, in ONE C call (st_eval_pool in include/signaltrain_hip.h).
        pool_x / pool_y: the concatenated audio on this engine's device, float32 or int16 (both the same; pool_y None: predict only); off / length: int64
        [nfiles], host arrays (tensors are read back to the host: the rows are formed there, and the device tables are kept from call to call
        while the arrays stay the same); knobs: [nfiles, K] (None for K == 0); batch: (file, window) rows per internal batch (default max_batch).
        Returns (stats, out): stats float64 [nfiles, 8] on the device (_lib.POOL_FIELDS; None without pool_y), out the pool-shaped float32 prediction,
        time-aligned with the input, zeros over each file's first L - y samples (None unless want_out or pool_y is None).  No host sync once the tables
        are known.  The engine keeps a workspace of its own for this: self.ws is not written; generation moves on."""
        dev = self.device
        pool_x = _recording("eval_pool", "pool_x", pool_x, dev, nonempty=True)
        if pool_y is not None:
            if not (torch.is_tensor(pool_y) and pool_y.shape == pool_x.shape and pool_y.device == dev and pool_y.dtype == pool_x.dtype):
                raise ValueError("eval_pool: pool_y must match pool_x in shape, dtype and device (or be None)")
            pool_y = _recording("eval_pool", "pool_y", pool_y, dev)
        want_out = bool(want_out or pool_y is None)
        d = self._infer_dims("eval_pool", batch)
        host = lambda t: np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.int64).reshape(-1)
        off_h, len_h = host(off), host(length)
        nfiles = int(len_h.size)
        if nfiles < 1 or off_h.size != nfiles:
            raise ValueError(f"eval_pool: off and length must hold one entry per file ({off_h.size} and {nfiles})")
        tables = self._kept("_pool_tables")     # the device tables and win_off: built once per (offsets, lengths, geometry) from the host lengths
        key = (off_h.tobytes(), len_h.tobytes(), d.L, d.y)
        if key not in tables:
            tables.clear()
            win = np.zeros(nfiles + 1, np.int64)
            rows = int(self.lib.st_eval_pool_rows(C.byref(d), len_h.ctypes.data_as(C.POINTER(C.c_longlong)), nfiles, win.ctypes.data_as(C.POINTER(C.c_longlong))))
            tables[key] = tuple(torch.from_numpy(a).to(dev) for a in (off_h, len_h, win)) + (rows,)
        off_d, len_d, win_d, rows = tables[key]
        kn, _ = _knob_rows("eval_pool", knobs, d.K, dev, (nfiles,), f" for {nfiles} files")
        ws = self._own_ws("eval_pool", "_pool_ws", d)
        stats = torch.empty(nfiles, _lib.POOL_STATS, dtype=torch.float64, device=dev) if pool_y is not None else None
        out = torch.empty(pool_x.numel(), dtype=torch.float32, device=dev) if want_out else None
        self.generation += 1
        self._call("st_eval_pool", C.byref(d), _lib.ptr(self.params), _pcm(pool_x),
                   C.c_void_p(pool_x.data_ptr()), None if pool_y is None else C.c_void_p(pool_y.data_ptr()), C.c_void_p(off_d.data_ptr()), C.c_void_p(len_d.data_ptr()),
                   C.c_void_p(win_d.data_ptr()), nfiles, rows, int(pool_x.numel()), _lib.ptr(kn), None if stats is None else C.c_void_p(stats.data_ptr()),
                   None if out is None else C.c_void_p(out.data_ptr()), _lib.ptr(ws), self._stream())
        return stats, out

    # ---------------------------------------------------------------- predict session: inference fed block by block
    def open_stream(self, channels=1, batch=None):
        """A predict session (st_predict_stream_* in include/signaltrain_hip.h): `channels` signals fed in lockstep block by block, every output sample
        emitted as soon as its window is complete.  batch: most (channel, window) rows per internal batch (default max_batch).  The session owns its history
        and workspace tensors, sized once here; self.ws and predict_long's workspace are not written.  RuntimeError on a geometry st_predict_supported rejects."""
        return PredictStream(self, channels, batch)

    def predict_channels(self, signal_2d, knobs, out=None, batch=None):
        """A resident [C, n] recording (float32 or int16) through the model, all channels in one session: one open_stream plus one final push.  knobs: [K] or
        [1, K] (all channels) or [C, K] (one setting per channel).  Returns [C, n - (L - y)] float32 on the device: row c is what predict_long gives for channel
        c, up to the order of the batches (1e-6).  On a geometry st_predict_supported rejects: one RuntimeWarning, then forward() window batch by window batch."""
        if not (torch.is_tensor(signal_2d) and signal_2d.dim() == 2 and signal_2d.shape[0] >= 1 and signal_2d.device == self.device
                and signal_2d.dtype in (torch.float32, torch.int16)):
            raise ValueError(f"predict_channels: signal must be a [C, n] float32 or int16 tensor on {self.device}")
        if self.predict_supported():
            key = (int(signal_2d.shape[0]), int(batch or self.max_batch), self.compute_dtype)
            kept = getattr(self, "_channel_stream", None)       # the last call's session: its history and workspace serve again, opened anew
            if kept is None or kept[0] != key:
                self._channel_stream = kept = (key, self.open_stream(key[0], key[1]))
            else:
                kept[1].reopen()
            return kept[1].push(signal_2d, knobs, final=True, out=out)
        global _warned_channels_unsupported
        if not _warned_channels_unsupported:
            _warned_channels_unsupported = True
            import warnings
            warnings.warn(f"signaltrain_amd: predict_channels does not run this geometry in a session (T={self.dims.T}, OT={self.dims.OT}: st_predict_supported); "
                          "taking the batched route, channel by channel", RuntimeWarning, stacklevel=2)
        C_, n = int(signal_2d.shape[0]), int(signal_2d.shape[1])
        L, y, K = self.dims.L, self.dims.y, self.dims.K
        n_out = max(n - (L - y), 0)
        sig = signal_2d.float() / 32767.0 if signal_2d.dtype == torch.int16 else signal_2d
        from .predict import _nwin
        nwin = _nwin(n, L, y)
        kn = _knob_rows("predict_channels", knobs, K, self.device, (1, C_), f": one row, or one per channel ({C_})")[0] if K else torch.zeros(1, 0, device=self.device)
        res = torch.empty(C_, n_out, dtype=torch.float32, device=self.device) if out is None else out
        bs = min(int(batch or self.max_batch), self.max_batch)
        for c in range(C_ if n_out else 0):
            padded = torch.zeros(L + (nwin - 1) * y, dtype=torch.float32, device=self.device)
            padded[:n] = sig[c]
            xw = padded.unfold(0, L, y)
            kc = kn[c if kn.shape[0] > 1 else 0].reshape(1, K)
            yc = torch.cat([self.forward(xw[b0:b0 + bs].contiguous(), kc.expand(min(bs, nwin - b0), K).contiguous())[0].reshape(-1) for b0 in range(0, nwin, bs)])
            res[c, :n_out] = yc[:n_out]
        return res[:, :n_out]

    # ---------------------------------------------------------------- encode once, decode at any knob setting
    def decode_supported(self):
        """Whether encode_long() / decode_long() run this geometry at this compute dtype (st_decode_supported; host arithmetic only)."""
        d = self.dims.with_batch(1)
        d.prec = _lib.PREC[self.compute_dtype]
        return bool(self.lib.st_decode_supported(C.byref(d)))

    def _geometry_key(self):
        return tuple(getattr(self.dims, k) for k in ("L", "N", "H", "T", "OT", "F", "K", "y"))

    def encode_long(self, signal, batch=None):
        """The knob-independent half of the model over a whole recording, once (st_encode_long in include/signaltrain_hip.h): window staging, the analysis GEMM, the
        polar form and encoder layers 1..4 of both autoencoders.  signal as predict_long takes it.  Returns a RecordingCode for decode_long() and
        fit_knobs(code=...); it is valid for this geometry, this compute dtype, this recording and the parameters as they are now -- that the parameters have not
        changed since the encode is the caller's precondition.  No host sync; self.ws is not written."""
        signal = _recording("encode_long", "signal", signal, self.device)
        d = self._infer_dims("encode_long", batch)
        ws = self._own_ws("encode_long", "_decode_ws", d)
        n = int(signal.numel())
        nwin = int(self.lib.st_predict_windows(C.byref(d), n))
        nbytes = int(self.lib.st_code_bytes(C.byref(d), n))
        code = torch.empty(max(nbytes, 16) // 4, dtype=torch.float32, device=self.device)
        if n > 0:
            self._call("st_encode_long", C.byref(d), _lib.ptr(self.params), _pcm(signal), C.c_void_p(signal.data_ptr()), n, _lib.ptr(code), _lib.ptr(ws), self._stream())
        return RecordingCode(code, signal, n, nwin, self._geometry_key(), self.compute_dtype)

    def _check_code(self, what, code):
        """A RecordingCode this engine can read: its geometry, compute dtype and device, the signal it holds as long as it says, the code as large as
        st_code_bytes asks for that length (a hand-built or truncated one must not reach the kernels)."""
        if not isinstance(code, RecordingCode):
            raise ValueError(f"{what}: code must be the RecordingCode encode_long() returned")
        if code.geometry != self._geometry_key():
            raise ValueError(f"{what}: the RecordingCode was built for another geometry ({code.geometry}, this engine has {self._geometry_key()})")
        if code.compute_dtype != self.compute_dtype:
            raise ValueError(f"{what}: the RecordingCode was built at compute dtype {code.compute_dtype!r}, this engine runs {self.compute_dtype!r}")
        if code.code.device != self.device or code.signal.device != self.device:
            raise ValueError(f"{what}: the RecordingCode lives on {code.code.device}, this engine on {self.device}")
        if int(code.signal.numel()) != code.n:
            raise ValueError(f"{what}: the RecordingCode was built from {code.n} samples, the signal it holds has {int(code.signal.numel())}")
        d = self.dims.with_batch(1)
        d.prec = _lib.PREC[self.compute_dtype]
        need = int(self.lib.st_code_bytes(C.byref(d), code.n))
        if code.code.dtype != torch.float32 or not code.code.is_contiguous() or int(code.code.numel()) * 4 != max(need, 16) or code.nwin != int(self.lib.st_predict_windows(C.byref(d), code.n)):
            raise ValueError(f"{what}: the RecordingCode holds {int(code.code.numel()) * 4} bytes in {code.nwin} windows; {code.n} samples need {need} bytes (st_code_bytes)")

    def decode_long(self, code, knobs, out=None, batch=None):
        """The recording behind `code` (encode_long) at one or several knob settings in ONE C call (st_decode_long): per setting only layers 5..9, the polar
        epilogue, the frames GEMM and the overlap-add run.  knobs: [K] (one setting; returns [n_out]), [S, K] (S settings) or [S, nwin, K] (S settings of one row
        per window); returns [S, n_out], row s what predict_long gives at setting s up to the order of a few sums.  out: a float32 device tensor [S, pitch] with
        pitch >= n_out, pitch % 4 == 0, 16-byte aligned rows, to write into.  batch need not be the batch of the encode.  No host sync; self.ws is not written."""
        self._check_code("decode_long", code)
        d = self._infer_dims("decode_long", batch)
        ws = self._own_ws("decode_long", "_decode_ws", d)
        n, nwin = code.n, code.nwin
        n_out = int(self.lib.st_predict_out_samples(C.byref(d), n))
        kn, single, S, rows = None, False, 1, 1
        if d.K:
            kn, single = _knob_settings("decode_long", knobs, d.K, nwin, n, self.device)
            S, rows = int(kn.shape[0]), int(kn.shape[1])
        pitch = (n_out + 3) // 4 * 4
        if out is None:
            out = torch.empty(S, pitch, dtype=torch.float32, device=self.device)
        elif not (out.dtype == torch.float32 and out.device == self.device and out.dim() == 2 and int(out.shape[0]) >= S and out.stride(1) == 1 and
                  out.stride(0) >= n_out and out.stride(0) % 4 == 0 and int(out.shape[1]) >= min(n_out, out.stride(0)) and out.data_ptr() % 16 == 0):
            raise ValueError(f"decode_long: out must be a 16-byte aligned float32 tensor [S >= {S}, >= {n_out}] on {self.device} with a row pitch that is a multiple of 4")
        if n_out > 0:
            self._call("st_decode_long", C.byref(d), _lib.ptr(self.params), _lib.ptr(code.code), _pcm(code.signal),
                       C.c_void_p(code.signal.data_ptr()), n, _lib.ptr(kn), rows, S, C.c_void_p(out.data_ptr()), int(out.stride(0)), _lib.ptr(ws), self._stream())
        y = out[:S, :n_out]
        return y[0] if single else y

    # ---------------------------------------------------------------- knob fit on the device
    def fit_knobs_supported(self):
        """Whether fit_knobs() runs this geometry (st_fit_knobs_supported: predict_supported() and at least one knob; host arithmetic only)."""
        return bool(self.lib.st_fit_knobs_supported(C.byref(self.dims.with_batch(1))))

    def _fit_args(self, what, first, signal, target, batch):
        """What every knob fit and score does in front of its knobs: signal (named `first` in the messages) and target in one format, the dims of a model
        that has knobs, the length and the window count."""
        signal, target = _recording_pair(what, signal, target, self.device, first)
        d = self._infer_dims(what, batch)
        if d.K < 1:
            raise ValueError(f"{what}: the model has no knobs")
        n = int(signal.numel())
        return d, signal, target, n, int(self.lib.st_predict_windows(C.byref(d), n))

    def fit_knobs(self, signal, target, knobs, steps=50, lr=0.05, betas=(0.9, 0.999), eps=1e-8, batch=None, state=None, want_grads=False):
        """The knob settings for which the model turns `signal` into `target`, fitted on the device in ONE C call (st_fit_knobs in include/signaltrain_hip.h):
        `steps` steps of Adam on J = mean over the n - (L - y) output samples of logcosh(y_hat - target), clamped to [-0.5, 0.5] after every step.  Output
        positions of the last window behind the recording's end carry no loss and no gradient (predict.fit_knobs' batched route counts its zero-padded tail);
        the two objectives coincide when n = L + k y.
        signal, target: 1-D float32 or int16 tensors of equal length on this engine's device (mixed dtypes: the int16 one is converted on the device, s / 32767);
        knobs: [K] (one setting) or [nwin, K] (one row per window), the start values -- cloned; batch: windows per internal batch (default max_batch);
        state: (m, v, first_step) as a previous call returned it, so that calls chain (default: zeros and step 1).
        Returns (knobs, loss_hist [steps] float64, grad_hist [steps, rows, K] or None, (m, v, next_step)), all on the device.  No host sync.  The engine keeps
        a workspace of its own for this (st_fit_knobs_ws_bytes, allocated on first use): self.ws and predict_long's workspace are not written.
        signal may also be the RecordingCode encode_long() returned for the recording (st_fit_knobs_coded): every step's forward then starts at layer 5 from
        the code -- no staging, no analysis GEMM, no encoder.  The parameters must not have changed since the encode."""
        code = None
        if isinstance(signal, RecordingCode):
            code = signal
            self._check_code("fit_knobs", code)
            signal = code.signal
        d, signal, target, n, nwin = self._fit_args("fit_knobs", "signal", signal, target, batch)
        steps = int(steps)
        kn, rows = _knob_rows("fit_knobs", knobs, d.K, self.device, (1, nwin), _per_window(nwin, n))
        kn = kn.clone()
        m, v, first = _adam_state(state, kn, self.device)
        ws = self._own_ws("fit_knobs", "_fit_ws", d)
        loss_hist = torch.zeros(max(steps, 0), dtype=torch.float64, device=self.device)
        grad_hist = torch.zeros(max(steps, 0), rows, d.K, dtype=torch.float32, device=self.device) if want_grads else None
        head = ("st_fit_knobs", C.byref(d), _lib.ptr(self.params)) if code is None else ("st_fit_knobs_coded", C.byref(d), _lib.ptr(self.params), _lib.ptr(code.code))
        self._call(*head, _pcm(signal), C.c_void_p(signal.data_ptr()), C.c_void_p(target.data_ptr()), n, _lib.ptr(kn), rows, _lib.ptr(m), _lib.ptr(v),
                   first, steps, float(lr), float(betas[0]), float(betas[1]), float(eps),
                   C.c_void_p(loss_hist.data_ptr()), _lib.ptr(grad_hist), _lib.ptr(ws), self._stream())
        shape = (d.K,) if (rows == 1 and torch.as_tensor(knobs).dim() == 1) else (rows, d.K)
        return kn.reshape(shape), loss_hist, grad_hist, (m, v, first + steps)

    # ---------------------------------------------------------------- many knob settings from one code
    def _multi_args(self, what, code, target, knobs, batch):
        """What score_knobs and fit_knobs_multi share: the code's validity (fit_knobs' checks), the recordings in one format, the settings as [S, rows, K] --
        cloned --, the dims and the workspace (st_knob_multi_ws_bytes, the engine's own)."""
        self._check_code(what, code)
        d, signal, target, n, nwin = self._fit_args(what, "the recording", code.signal, target, batch)
        kn = _knob_settings(what, knobs, d.K, nwin, n, self.device, strict=True)[0].clone()
        S = int(kn.shape[0])
        return d, signal, target, kn, S, n, nwin, self._own_ws(what, "_multi_ws", d, S)

    def score_knobs(self, code, target, knobs, batch=None, per_window=False):
        """J = mean log-cosh of (model output - target) of the recording behind `code` (encode_long) at S knob settings, in ONE C call (st_score_knobs_coded in
        include/signaltrain_hip.h): per setting only the decoder forward, the frames GEMM and one overlap-add that keeps nothing but the loss partials run -- no
        [S, n_out] output exists.  knobs: [S, K], or [S, nwin, K] for one row per window.  Returns loss [S] float64 on the device; per_window=True: (loss,
        win_loss [S, nwin] float32), win_loss[s, w] window w's share of loss[s].  A recording of at most half a batch is stacked: rows of a batch are
        (setting, window) pairs (st_knob_multi_plan).  The code must be valid (fit_knobs' checks; that the parameters have not changed is the caller's
        precondition).  No host sync; self.ws is not written."""
        d, signal, target, kn, S, n, nwin, ws = self._multi_args("score_knobs", code, target, knobs, batch)
        loss = torch.zeros(S, dtype=torch.float64, device=self.device)
        win = torch.zeros(S, nwin, dtype=torch.float32, device=self.device) if per_window else None
        self._call("st_score_knobs_coded", C.byref(d), _lib.ptr(self.params), _lib.ptr(code.code), _pcm(signal), C.c_void_p(signal.data_ptr()),
                   C.c_void_p(target.data_ptr()), n, _lib.ptr(kn), int(kn.shape[1]), S, C.c_void_p(loss.data_ptr()), _lib.ptr(win), _lib.ptr(ws), self._stream())
        return (loss, win) if per_window else loss

    def fit_knobs_multi(self, code, target, knobs, steps=50, lr=0.05, betas=(0.9, 0.999), eps=1e-8, batch=None, state=None, want_grads=False):
        """fit_knobs from S starts at once, in ONE C call (st_fit_knobs_multi_coded): S independent Adam runs on the objective of fit_knobs, each with its own
        knob rows, moments, loss history and gradient history, from the recording's code.  knobs: [S, K] or [S, nwin, K], the start values -- cloned; state:
        (m, v, first_step) as a previous call returned it, so that calls chain (default: zeros and step 1), as fit_knobs.  Returns (knobs [S, ...] in the shape
        given, loss_hist [steps, S] float64, (m, v, next_step)) and, with want_grads=True, grads [steps, S, rows, K] behind them.  A recording of at most half a
        batch is stacked: rows of a batch are (setting, window) pairs (st_knob_multi_plan).  No host sync; self.ws is not written."""
        d, signal, target, kn, S, n, nwin, ws = self._multi_args("fit_knobs_multi", code, target, knobs, batch)
        steps = int(steps)
        rows = int(kn.shape[1])
        m, v, first = _adam_state(state, kn, self.device)
        loss_hist = torch.zeros(max(steps, 0), S, dtype=torch.float64, device=self.device)
        grads = torch.zeros(max(steps, 0), S, rows, d.K, dtype=torch.float32, device=self.device) if want_grads else None
        self._call("st_fit_knobs_multi_coded", C.byref(d), _lib.ptr(self.params), _lib.ptr(code.code), _pcm(signal), C.c_void_p(signal.data_ptr()),
                   C.c_void_p(target.data_ptr()), n, _lib.ptr(kn), rows, S, _lib.ptr(m), _lib.ptr(v), first, steps, float(lr), float(betas[0]), float(betas[1]),
                   float(eps), C.c_void_p(loss_hist.data_ptr()), _lib.ptr(grads), _lib.ptr(ws), self._stream())
        shape = tuple(torch.as_tensor(knobs).shape)
        res = (kn.reshape(shape), loss_hist, (m.reshape(shape), v.reshape(shape), first + steps))
        return res + (grads,) if want_grads else res

    # ---------------------------------------------------------------- the step as one HIP graph
    def graph_capture(self, batch, lr_table, betas=(0.9, 0.999), eps=1e-8):
        """Capture st_train_step for `batch` windows into a HIP graph (st_graph_create).  The step counter and the learning rate
        live on the device (scalars[6], scalars[7]; `lr_table` = the 1-cycle table, uploaded once): graph_step() then needs no
        per-step arguments.  The minibatch is read from the fixed buffers self.gx / self.gk / self.gy."""
        self._refuse_frozen("graph_capture")
        d = self._dims(int(batch))
        dev = self.device
        self.gx = torch.zeros(d.B, d.L, dtype=torch.float32, device=dev)
        self.gk = torch.zeros(d.B, d.K, dtype=torch.float32, device=dev) if d.K else None      # K = 0: NULL (see _prep)
        self.gy = torch.zeros(d.B, d.y, dtype=torch.float32, device=dev)
        self.g_lr = torch.as_tensor(np.asarray(lr_table, dtype=np.float32), device=dev).contiguous()
        self.scalars[6] = float(self.step_count)
        self._graph_dims = d
        handle = C.c_void_p()
        side = torch.cuda.Stream(device=dev)             # capture needs a non-default stream
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.device(dev):
            _lib.check(self.lib.st_graph_create(C.byref(d), _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self.m), _lib.ptr(self.v),
                                                _lib.ptr(self.gx), _lib.ptr(self.gk), _lib.ptr(self.gy), _lib.ptr(self.ws), _lib.ptr(self.scalars),
                                                _lib.ptr(self.g_lr), int(self.g_lr.numel()), float(betas[0]), float(betas[1]), float(eps),
                                                C.c_void_p(side.cuda_stream), C.byref(handle)), "st_graph_create")
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = handle
        return handle

    def graph_step(self, x=None, knobs=None, y=None):
        """One optimisation step = one hipGraphLaunch on the current stream.  x / knobs / y (optional) are copied into the
        graph's input buffers first; with all three None the buffers are used as they are (device-resident data)."""
        self._refuse_frozen("graph_step")
        if x is not None:
            self.gx.copy_(x); self.gy.copy_(y)
            if self.dims.K: self.gk.copy_(knobs)
        self.step_count += 1; self.generation += 1
        self._call("st_graph_launch", self.graph, self._stream())
        return self.scalars

    def graph_destroy(self):
        if getattr(self, "graph", None) is not None:
            self._call("st_graph_destroy", self.graph); self.graph = None

    def dp_train_step(self, x, knobs, y, lr, betas=(0.9, 0.999), eps=1e-8, force_exchange=False, split_last=False, pack16=False):
        """The data-parallel step driven from C (st_dp_train_step): this rank's shard, both gradient buckets all-reduced on the
        library's RCCL communicator under the backward, clip after the reduction, replicated Adam.  split_last: the last exchange by basis
        (only 2.1 MB exposed); pack16: that exchange on bfloat16 values (the *_all arithmetic modes only)."""
        d, x, knobs, y = self._prep(x, knobs, y)
        self.step_count += 1; self.generation += 1; self.lr = float(lr)
        self._call("st_dp_train_step", self.dp, C.byref(d), _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self.m),
                   _lib.ptr(self.v), _lib.ptr(self._stage_buf()), _lib.ptr(x), _lib.ptr(knobs), _lib.ptr(y), _lib.ptr(self.ws),
                   _lib.ptr(self.scalars), float(lr), float(betas[0]), float(betas[1]), float(eps),
                   int(self.step_count), (1 if force_exchange else 0) | (2 if split_last else 0) | (4 if pack16 else 0), self._stream())
        return self.scalars

    def clip_adam(self, lr, grad_scale=1.0, betas=(0.9, 0.999), eps=1e-8):
        """L1 clip + Adam on the current self.grads (data parallel: call after the all-reduce with
        grad_scale = 1/world; the norm is recomputed on the reduced gradient, identically on all ranks)."""
        self.step_count += 1; self.lr = float(lr)
        d = self._pending[0] if self._pending is not None else self._dims(self.dims.B)     # the STEP's dims: its partial-sum counts carve the workspace
        self._call("st_dp_clip_adam", C.byref(d), _lib.ptr(self.params), _lib.ptr(self.grads),
                   _lib.ptr(self.m), _lib.ptr(self.v), _lib.ptr(self.ws), _lib.ptr(self.scalars),
                   float(grad_scale), float(lr), float(betas[0]), float(betas[1]), float(eps),
                   int(self.step_count), self._stream())
        return self.scalars

    def loss(self):
        """Host copy of the last loss (device->host sync; the reference does this every 10 iterations)."""
        return float(self.scalars[0].item())

    def overflow_steps(self, reset=True):
        """Steps skipped so far because a gradient overflowed under the loss scale (scalars[5]; device->host sync).  The
        caller's loss-scale policy (train.train halves the scale, like Apex's dynamic scaler) acts on it."""
        n = int(self.scalars[5].item())
        if reset and n:
            self.scalars[5] = 0.0
        return n
