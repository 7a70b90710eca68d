"""GPU: the train step with frozen parameter groups (st_train_step_groups) and the Python surface over it.

Geometries: the smallest shapes that reach each autoencoder backward route --
  default   st_geometry(1, 4), B = 3        fp32 kept-activation ae_bwd (its NOIN instantiation where the analysis bases are frozen), 128-row-tile GEMMs, weight images
  n256      row n256, B = 3                 fused, recompute sizes
  wide      row t33_ot17, B = 3             the wide autoencoder path
  bf16      default geometry, B = 4, bf16_all   the split 16-bit backward
  f16       row n384, B = 4, f16_all        clip_all = 1 and a loss scale
Every case starts from the state one full st_train_step leaves (non-zero moments) and compares at step 2.  The full step and st_loss_backward of a case
run once and are shared."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from oracle import st_oracle as O
from signaltrain_amd import _lib
from signaltrain_amd.engine import StepEngine
from tests import dims_table as D
from tests import frozen_groups_rule as R
from tests import gpu_checks as G

pytestmark = pytest.mark.gpu

GEOS = {"default": (None, 3, "f32"), "n256": ("n256", 3, "f32"), "wide": ("t33_ot17", 3, "f32"), "bf16": (None, 4, "bf16_all"), "f16": ("n384", 4, "f16_all")}
MASKS = (12, 14, 13, 3, 4, 8)
LR = 1e-3
ST_ERR_ARG = -1


class Case:
    def __init__(self, gid):
        row, B, dtype = GEOS[gid]
        geo = O.geometry(1, 4) if row is None else D.geo_of(row)
        self.geo, self.X, self.Y, self.KN, self.P = G.make_case(B=B, seed=1, K=4, geo=geo)
        self.eng = StepEngine(G.dims_of(geo, B, 4), G.DEV, compute_dtype=dtype)      # f16_all: loss scale 4096 and the clip over all parameters by default
        self.d = self.eng._dims(B)
        self.inv_s = np.float32(1.0 / self.eng.loss_scale)
        self.clip_all = bool(self.eng.clip_all)
        self.x, self.y, self.kn = G.t(self.X), G.t(self.Y), G.t(self.KN)
        self.offs = list(self.eng.layout.offsets) + [self.eng.layout.total]
        self.bounds = [self.offs[0], self.offs[2], self.offs[4], self.offs[22], self.offs[40]]
        e = self.eng
        e.load_state_dict(self.P)
        e.m.zero_(); e.v.zero_(); e.grads.zero_(); e.scalars.zero_()
        self.call("st_train_step", 1)
        self.state = {k: getattr(e, k).clone() for k in ("params", "m", "v", "grads", "scalars")}      # after step 1: where every comparison starts
        self.full = self.run("st_train_step", 2)
        self.restore()
        e.loss_backward(self.x, self.kn, self.y)
        torch.cuda.synchronize()
        self.lb = e.grads.clone(); self.lb_scalars = e.scalars.clone()

    def rng(self, g):
        return slice(self.bounds[g], self.bounds[g + 1])

    def restore(self):
        for k, v in self.state.items():
            getattr(self.eng, k).copy_(v)

    def call(self, name, step, mask=None, expect=0, step_ptr=True, lr=LR):
        e, d = self.eng, self.d
        head = (C.byref(d), _lib.ptr(e.params), _lib.ptr(e.grads), _lib.ptr(e.m), _lib.ptr(e.v), _lib.ptr(self.x), _lib.ptr(self.kn), _lib.ptr(self.y),
                _lib.ptr(e.ws), _lib.ptr(e.scalars), float(lr), 0.9, 0.999, 1e-8)
        if name == "st_train_step":
            rc = e.lib.st_train_step(*head, int(step), G.stream())
        else:
            steps = (C.c_int * 4)(*([step] * 4 if np.isscalar(step) else step)) if step_ptr else None
            rc = e.lib.st_train_step_groups(*head, steps, int(mask), G.stream())
        torch.cuda.synchronize()
        assert rc == expect, (name, rc, e.lib.st_last_error())
        return rc

    def run(self, name, step, mask=None, poison=False):
        """From the shared state: the call, and clones of what it left.  poison: m, v and grads of the frozen groups hold a NaN pattern beforehand."""
        self.restore()
        e = self.eng
        if poison:
            nan = torch.tensor(0x7FC0BEEF, dtype=torch.int32, device=G.DEV).view(torch.float32)
            for g in range(4):
                if not (mask >> g) & 1:
                    for buf in (e.m, e.v, e.grads):
                        buf[self.rng(g)] = nan
        before = {k: getattr(e, k).clone() for k in ("params", "m", "v")}
        self.call(name, step, mask)
        out = {k: getattr(e, k).clone() for k in ("params", "m", "v", "grads", "scalars")}
        out["before"] = before
        return out


@functools.lru_cache(maxsize=None)
def case(gid):
    return Case(gid)


@functools.lru_cache(maxsize=None)
def masked(gid, mask):
    return case(gid).run("st_train_step_groups", 2, mask, poison=True)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("gid", list(GEOS))
def test_mask_15_with_equal_steps_is_the_full_step(gid):
    c = case(gid)
    got = c.run("st_train_step_groups", 2, 15)
    for k in ("params", "grads", "m", "v", "scalars"):
        assert torch.equal(bits(got[k]), bits(c.full[k])), (gid, k)
    assert not torch.equal(bits(got["params"]), bits(c.state["params"]))


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("gid", list(GEOS))
def test_frozen_ranges_are_not_touched(gid, mask):
    c, r = case(gid), masked(gid, mask)
    for g in range(4):
        s = c.rng(g)
        if (mask >> g) & 1:
            assert not torch.equal(bits(r["params"][s]), bits(r["before"]["params"][s])), (gid, mask, g)      # a trainable group moved
            assert torch.isfinite(r["m"][s]).all() and torch.isfinite(r["v"][s]).all() and torch.isfinite(r["params"][s]).all()
        else:
            for k in ("params", "m", "v"):
                assert torch.equal(bits(r[k][s]), bits(r["before"][k][s])), (gid, mask, g, k)
            assert torch.isnan(r["m"][s]).all() and torch.isnan(r["v"][s]).all()
    assert torch.isfinite(r["scalars"]).all()


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("gid", list(GEOS))
def test_trainable_gradients_are_those_of_the_full_backward(gid, mask):
    """Bit for bit: st_loss_backward's range, times the reported coefficient (and the exact power-of-two unscale of a loss scale) in float32 where the
    optimizer rescales in place, as it is elsewhere.  The skipped work feeds none of these sums."""
    c, r = case(gid), masked(gid, mask)
    coef = np.float32(r["scalars"][4].item())
    for g in range(4):
        if not (mask >> g) & 1:
            continue
        s = c.rng(g)
        clipped = g < 2 or c.clip_all
        sc = np.float32(c.inv_s * coef) if clipped else c.inv_s          # clip_adam's sc = grad_scale * coef, one float32 product
        ref = c.lb[s] if sc == np.float32(1.0) else c.lb[s] * torch.tensor(sc, device=G.DEV)
        same = torch.equal(bits(r["grads"][s]), bits(ref))
        if not same:
            dd = (r["grads"][s] - ref).abs().max().item()
            print(f"FROZEN_GRAD_DIFF | {gid} | mask {mask} | group {g} | max abs {dd:.3e} of {ref.abs().max().item():.3e}")
        assert same, (gid, mask, g)


def _l1(c, groups):
    return sum(float((c.lb[c.rng(g)].double() * float(c.inv_s)).abs().sum().item()) for g in groups)


@pytest.mark.parametrize("gid", list(GEOS))
def test_clip_norm_runs_over_the_trainable_tensors_of_the_scope(gid):
    c = case(gid)
    for mask in (14, 12, 13, 3, 8):
        sc = masked(gid, mask)["scalars"].cpu().numpy()
        groups = [g for g in range(4) if (mask >> g) & 1 and (g < 2 or c.clip_all)]
        want = _l1(c, groups)
        print(f"FROZEN_NORM | {gid} | mask {mask} | got {sc[3]:.6e} want {want:.6e} coef {sc[4]:.6e}")
        if not groups:
            assert sc[3] == 0.0 and sc[4] == 1.0, (gid, mask, sc)
        else:
            assert abs(sc[3] - want) <= 1e-3 * want, (gid, mask, sc[3], want)
            assert abs(sc[4] - min(1.0, 1.0 / (want + 1e-6))) <= 1e-3 * sc[4]
        for k in (0, 1, 2, 5):                    # loss terms and the overflow count: the full step's
            assert sc[k] == c.full["scalars"][k].item(), (gid, mask, k)
    if gid == "f16":
        assert c.clip_all and masked(gid, 12)["scalars"][3].item() > 0          # the autoencoder gradients' norm
    else:
        assert masked(gid, 12)["scalars"][3].item() == 0.0 and masked(gid, 12)["scalars"][4].item() == 1.0


@pytest.mark.parametrize("gid", ["n256", "default"])
def test_per_group_steps_follow_the_oracle_rule(gid):
    """Two steps with the front end frozen, two with everything trainable at steps {1, 1, 3, 3} and {2, 2, 4, 4}: the parameters against the numpy rule
    of tests/test_frozen_groups_host.py in float32, at the 2e-5 absolute of dims_table.condition_bound for parameters after a train step -- a bound that
    belongs to the learning rate gpu_checks._run_fused steps with (the head of its 1-cycle table), which is the rate used here."""
    c, e = case(gid), case(gid).eng
    lr = float(O.get_1cycle_schedule(lr_max=1e-3, n_data_points=200, epochs=1, batch_size=2)[0][0])
    e.load_state_dict(c.P); e.m.zero_(); e.v.zero_(); e.grads.zero_(); e.scalars.zero_()
    Pq = {k: c.P[k].copy() for k in O.param_order()}
    M = {k: np.zeros_like(v) for k, v in Pq.items()}; V = {k: np.zeros_like(v) for k, v in Pq.items()}
    try:
        for it, (mask, steps) in enumerate(((12, (0, 0, 1, 1)), (12, (0, 0, 2, 2)), (15, (1, 1, 3, 3)), (15, (2, 2, 4, 4)))):
            c.call("st_train_step_groups", list(steps), mask, lr=lr)
            _, Gq, _ = O.model_loss_bwd(c.X, c.KN, c.Y, Pq, c.geo)
            R.apply_step(Pq, M, V, Gq, mask, steps, lr)
            got = e.state_dict()
            worst = max((float(np.abs(got[k].cpu().numpy().reshape(Pq[k].shape) - Pq[k]).max()), k) for k in Pq)
            print(f"FROZEN_STEPS | {gid} | step {it} mask {mask} | worst |dp| {worst[0]:.3e} at {worst[1]}")
            assert worst[0] < 2e-5, (gid, it, worst)
            if mask == 12:
                for k in O.STFT_KEYS:
                    assert np.array_equal(got[k].cpu().numpy().reshape(c.P[k].shape), c.P[k]), (it, k)
    finally:
        c.restore()


def _profile_names(c, mask, steps=2):
    lib = c.eng.lib
    c.restore()
    assert lib.st_profile_enable(1) == 0
    try:
        c.call("st_train_step_groups", steps, mask)
        buf = C.create_string_buffer(1 << 14)
        assert lib.st_profile_report(buf, len(buf)) == 0
    finally:
        lib.st_profile_enable(0)
    return [ln.split()[0] for ln in buf.value.decode().splitlines() if ln.strip()]


@pytest.mark.parametrize("gid", ["default", "wide", "bf16"])
def test_a_stage_outside_the_set_issues_no_launch(gid):
    c, lib = case(gid), case(gid).eng.lib
    seen = {}
    for mask in range(1, 16):
        names = seen[mask] = _profile_names(c, mask, steps=[2, 3, 2, 2] if mask == 15 else 2)      # mask 15 with one step number is the plain step
        st = lib.st_step_groups_stages(mask)
        assert st == R.stages_of(mask)
        has = lambda n: n in names
        assert has("analysis_wgrad") == has("analysis_wgrad_reduce") == bool(st & _lib.STAGE_ANA_WGRAD), (mask, names)
        assert has("synthesis_wgrad") == bool(st & _lib.STAGE_SYN_WGRAD), (mask, names)
        assert has("synthesis_dgrad") == bool(st & _lib.STAGE_SYN_DGRAD), (mask, names)
        assert any(has(n) for n in ("ae_bwd", "ae_bwd_dec", "ae_wide_bwd", "ae_wide_bwd_noin")) == bool(st & _lib.STAGE_AE_BWD), (mask, names)
        # the polar backward rides in post_ae (fused geometries) / closes ae_wide_bwd (wide ones); without it those launches carry other names
        assert (has("post_ae") or has("ae_wide_bwd")) == bool(st & _lib.STAGE_AE_DINPUT), (mask, names)
        if (st & _lib.STAGE_AE_BWD) and not (st & _lib.STAGE_AE_DINPUT):
            assert has("post_ae_reduce") or has("ae_wide_bwd_noin"), (mask, names)
        assert has("synthesis_wgrad_reduce") == (mask == 2), (mask, names)      # alone, the synthesis slabs are summed by their own launch
        assert has(f"clip_adam_g{mask}") and not has("clip_adam"), (mask, names)      # the optimizer launch names exactly the groups it updates
        assert has("prep") and has("analysis_fwd") and (has("ae_fwd") or has("ae_wide_fwd")) and has("ola_loss"), names
    assert not any(n.startswith("analysis_wgrad") or n.startswith("synthesis_wgrad") or n in ("post_ae", "ae_wide_bwd") for n in seen[12])
    assert "synthesis_wgrad" in seen[14] and not any(n.startswith("analysis_wgrad") for n in seen[14])
    assert "clip_adam_g3" in seen[3]
    c.restore()
    lib.st_profile_enable(1)
    try:
        c.call("st_train_step_groups", 2, 15)
        buf = C.create_string_buffer(1 << 14); lib.st_profile_report(buf, len(buf))
    finally:
        lib.st_profile_enable(0)
    assert "clip_adam" in [ln.split()[0] for ln in buf.value.decode().splitlines()]


def test_refusals_name_the_rule_and_launch_nothing():
    c = case("n256")
    c.restore()
    p0 = c.eng.params.clone()
    for kw, word in ((dict(step=2, mask=0), b"trainable"), (dict(step=2, mask=16), b"trainable"), (dict(step=[2, 2, 0, 2], mask=12), b"step[2]"),
                     (dict(step=2, mask=12, step_ptr=False), b"null pointer")):
        rc = c.call("st_train_step_groups", expect=ST_ERR_ARG, **kw)
        assert rc == ST_ERR_ARG and word in c.eng.lib.st_last_error(), (kw, c.eng.lib.st_last_error())
        assert torch.equal(bits(c.eng.params), bits(p0))
    c.call("st_train_step_groups", [0, 0, 2, 2], 12)          # a frozen group's entry is ignored
    assert not torch.equal(bits(c.eng.params), bits(p0))
    c.restore()


# ------------------------------------------------------------------------------------------------ module level
def _model_and_batch(B=4):
    from signaltrain_amd import nn_proc
    nn_proc._QUIET = True
    torch.manual_seed(3)
    model = nn_proc.st_model(scale_factor=1, shrink_factor=4, num_knobs=4).to(G.DEV)
    geo = O.geometry(1, 4)
    X, Y, KN = O.synth_comp4c_batch(B, geo["L"], geo["y"], np.random.default_rng(5))
    return model, G.t(X), G.t(Y), G.t(KN)


def _moved(sd0, sd1):
    return {k for k in sd0 if not torch.equal(sd0[k], sd1[k])}


def test_model_freeze_keeps_the_front_end_bit_for_bit():
    from signaltrain_amd.engine import STFT_KEYS
    model, x, y, kn = _model_and_batch()
    eng = model.engine(x)
    model.freeze()
    assert eng.trainable == 12
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for _ in range(3):
        eng.train_step(x, kn, y, LR)
    torch.cuda.synchronize()
    moved = _moved(sd0, model.state_dict())
    assert not moved & set(STFT_KEYS) and moved == set(sd0) - set(STFT_KEYS), sorted(moved)
    assert eng.group_steps == [0, 0, 3, 3] and eng.step_count == 3
    osd = eng.optimizer_state_dict()
    assert [float(osd["state"][i]["step"]) for i in (0, 2, 4, 22)] == [0.0, 0.0, 3.0, 3.0]
    model.unfreeze()
    assert eng.trainable == 15
    eng.train_step(x, kn, y, LR)               # the bases start at Adam step 1, the autoencoders are at 4
    assert eng.group_steps == [1, 1, 4, 4]
    assert set(STFT_KEYS) <= _moved(sd0, model.state_dict())
    eng2 = StepEngine(eng.dims, G.DEV)
    assert eng2.load_optimizer_state_dict(eng.optimizer_state_dict()) is not None
    assert eng2.group_steps == [1, 1, 4, 4] and eng2.step_count == 4 and torch.equal(eng2.m, eng.m) and torch.equal(eng2.v, eng.v)


def test_freeze_layers_freezes_one_autoencoder():
    from signaltrain_amd import nn_proc
    model, x, y, kn = _model_and_batch()
    eng = model.engine(x)
    nn_proc.freeze_layers([model.mpaec.aenc])
    assert eng.sync_trainable(model) == 1 | 2 | 8
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    eng.train_step(x, kn, y, LR)
    torch.cuda.synchronize()
    moved = _moved(sd0, model.state_dict())
    assert moved == {k for k in sd0 if ".aenc." not in k}, sorted(set(sd0) - moved)


def test_data_parallel_refuses_frozen_groups():
    from signaltrain_amd.dp import DataParallel
    model, x, y, kn = _model_and_batch()
    eng = model.engine(x)
    dp = DataParallel(eng, force_collectives=True)
    try:
        model.freeze()
        p0 = eng.params.clone()
        with pytest.raises(NotImplementedError, match="frozen"):
            dp.train_step(x, kn, y, LR)
        assert torch.equal(eng.params, p0)
        with pytest.raises(NotImplementedError, match="frozen"):      # ... and so does the captured step
            eng.graph_capture(x.shape[0], [LR, LR])
    finally:
        dp.close()


def test_train_driver_two_phase_schedule(tmp_path, monkeypatch):
    """train.train(freeze=("frontend",), unfreeze_epoch=1, epochs=2): the bases change only in the second epoch."""
    from signaltrain_amd import audio, nn_proc, train
    from signaltrain_amd.engine import STFT_KEYS
    nn_proc._QUIET = True
    snaps = []
    loop, evals = train.train_loop, train.eval_status_save

    def loop_spy(model, *a, **kw):
        snaps.append({k: v.detach().clone() for k, v in model.state_dict().items()})
        return loop(model, *a, **kw)

    def eval_spy(model, *a, **kw):
        torch.cuda.synchronize()
        snaps.append({k: v.detach().clone() for k, v in model.state_dict().items()})
        return evals(model, *a, **kw)

    monkeypatch.setattr(train, "train_loop", loop_spy); monkeypatch.setattr(train, "eval_status_save", eval_spy)
    monkeypatch.chdir(tmp_path)
    model = train.train(effect=audio.Compressor_4c(), epochs=2, n_data_points=64, batch_size=16, device=torch.device(G.DEV), num_workers=0,
                        freeze=("frontend",), unfreeze_epoch=1)
    assert len(snaps) == 3                       # before the loop, after epoch 0, after epoch 1
    first, second = _moved(snaps[0], snaps[1]), _moved(snaps[1], snaps[2])
    assert not first & set(STFT_KEYS) and first, sorted(first)
    assert set(STFT_KEYS) <= second
    eng = model.engine(torch.zeros(16, 8192, device=G.DEV))
    assert eng.trainable == 15 and eng.group_steps == [4, 4, 8, 8] and all(p.requires_grad for p in model.parameters())
    assert os.path.isfile("modelcheckpoint.tar")
