"""Host side of the frozen parameter groups (st_train_step_groups; nn_proc.freeze_layers / st_model.freeze; train.train(freeze=...)): runs without a GPU.

- st_step_groups_stages against the stage rule, written out here as a table;
- the oracle's rule for such a step (tests/frozen_groups_rule.py, which the GPU tests hold the device to) IS torch's: requires_grad = False parameters
  under clip_grad_norm_ + torch.optim.Adam, two steps with the front end frozen and two with everything trainable;
- the optimizer state with per-group step numbers round-trips through misc.adam_state_dict / flatten_optimizer_state and continues a torch.optim.Adam;
- sync_trainable's and train()'s refusals."""
import numpy as np
import pytest
import torch

from oracle import st_oracle as O
from signaltrain_amd import _lib, misc
from tests import dims_table as D
from tests import frozen_groups_rule as R

# mask -> stages (SYN_DGRAD 1 | SYN_WGRAD 2 | AE_BWD 4 | AE_DINPUT 8 | ANA_WGRAD 16), every mask spelled out
STAGES = {
    1: 1 | 4 | 8 | 16,             # analysis alone: everything behind it runs, the synthesis weight gradient does not
    2: 2,                          # synthesis alone: its weight gradient and nothing else
    3: 1 | 2 | 4 | 8 | 16,
    4: 1 | 4,                      # one autoencoder: the data gradient into both nets, their backward, no input gradient
    5: 1 | 4 | 8 | 16,
    6: 1 | 2 | 4,
    7: 1 | 2 | 4 | 8 | 16,
    8: 1 | 4,
    9: 1 | 4 | 8 | 16,
    10: 1 | 2 | 4,
    11: 1 | 2 | 4 | 8 | 16,
    12: 1 | 4,                     # the front end frozen
    13: 1 | 4 | 8 | 16,            # synthesis frozen
    14: 1 | 2 | 4,                 # analysis frozen
    15: 1 | 2 | 4 | 8 | 16,
}


def test_stage_rule_for_every_mask():
    lib = _lib.load()
    assert (_lib.STAGE_SYN_DGRAD, _lib.STAGE_SYN_WGRAD, _lib.STAGE_AE_BWD, _lib.STAGE_AE_DINPUT, _lib.STAGE_ANA_WGRAD) == (1, 2, 4, 8, 16)
    for mask, want in STAGES.items():
        assert lib.st_step_groups_stages(mask) == want, (mask, lib.st_step_groups_stages(mask), want)
        assert R.stages_of(mask) == want, mask
    for bad in (0, 16, -1):
        assert lib.st_step_groups_stages(bad) < 0, bad


def _case():
    geo = D.geo_of("n32")
    rng = np.random.default_rng(11)
    from tests.golden_util import perturb_stft
    P = O.init_params(geo, 4, rng); perturb_stft(P, seed=5)
    X, Y, KN = O.synth_comp4c_batch(2, geo["L"], geo["y"], rng)
    return geo, P, X, Y, KN


def test_oracle_rule_is_torch_requires_grad_false():
    """Two steps with the front end frozen (mask 12), then two with everything trainable (the groups then at steps 1, 1, 3, 3 and 2, 2, 4, 4): every
    parameter after every step at the tolerance of test_abi_and_host.py::test_cpu_port_matches_oracle (2e-5 absolute; the loss 3e-5 relative), the frozen
    tensors exactly."""
    from oracle import torch_cpu_step as T
    geo, P, X, Y, KN = _case()
    f = np.float64
    lr = 1e-3
    keys = R.group_keys()
    # torch side: float64 on the CPU, the forward of oracle/torch_cpu_step.py
    Pt = {k: torch.from_numpy(P[k].astype(f)).requires_grad_(True) for k in O.param_order()}
    opt = torch.optim.Adam(list(Pt.values()), lr=lr, weight_decay=0)
    x, y, kn = (torch.from_numpy(a.astype(f)) for a in (X, Y, KN))
    # oracle side
    Pq = {k: P[k].copy() for k in O.param_order()}
    M = {k: np.zeros_like(v) for k, v in Pq.items()}; V = {k: np.zeros_like(v) for k, v in Pq.items()}
    steps = [0, 0, 0, 0]
    P0 = {k: v.copy() for k, v in Pq.items()}
    for it, mask in enumerate((12, 12, 15, 15)):
        for g, ks in enumerate(keys):
            for k in ks:
                Pt[k].requires_grad_(bool(mask & R.GROUP_BITS[g]))
        y_hat, mag, mag_hat = T.forward(Pt, x, kn, N=geo["N"], H=geo["H"])
        Fb = mag_hat.shape[-1]
        sbf = torch.exp((7. / Fb) * torch.arange(0., Fb, dtype=torch.float64)).expand_as(mag_hat)
        loss = torch.mean(torch.log(torch.cosh(y - y_hat))) + 2e-5 / 10 * torch.abs(mag_hat * sbf).mean()
        opt.zero_grad()
        loss.backward()
        with_grad = [Pt[k] for k in O.STFT_KEYS if Pt[k].grad is not None]
        assert len(with_grad) == (0 if mask == 12 else 4)
        torch.nn.utils.clip_grad_norm_(with_grad, max_norm=1., norm_type=1)
        opt.step()

        steps = [s + 1 if mask & R.GROUP_BITS[g] else s for g, s in enumerate(steps)]
        lo, Gq, _ = O.model_loss_bwd(X.astype(f), KN.astype(f), Y.astype(f), {k: v.astype(f) for k, v in Pq.items()}, geo)
        norm, coef = R.apply_step(Pq, M, V, Gq, mask, steps, lr)
        if mask == 12:
            assert (norm, coef) == (0.0, 1.0)
        assert abs(float(loss.item()) - lo) <= 3e-5 * abs(lo), (it, float(loss.item()), lo)
        for g, ks in enumerate(keys):
            for k in ks:
                got, ref = Pq[k], Pt[k].detach().numpy()
                assert np.abs(got - ref).max() < 2e-5, (it, k)
                if it < 2 and g < 2:          # frozen: not a bit moved, on either side
                    assert np.array_equal(got, P0[k]) and np.array_equal(ref, P0[k].astype(f)), (it, k)
                    assert not M[k].any() and not V[k].any() and Pt[k] not in opt.state
                else:
                    assert not np.array_equal(got, P0[k]), (it, k)
    assert steps == [2, 2, 4, 4]
    assert [int(opt.state[Pt[ks[0]]]["step"]) for ks in keys] == [2, 2, 4, 4]


def _adam_with_state(shapes, steps_per_group, seed):
    rng = np.random.default_rng(seed)
    ps = [torch.from_numpy(rng.standard_normal(s).astype(np.float32)).requires_grad_(True) for s in shapes]
    opt = torch.optim.Adam(ps, lr=1e-3)
    for g, sl in enumerate(misc.GROUP_SLICES):
        for p in ps[sl]:
            if steps_per_group[g]:
                opt.state[p] = {"step": torch.tensor(float(steps_per_group[g])),
                                "exp_avg": torch.from_numpy(0.1 * rng.standard_normal(p.shape).astype(np.float32)),
                                "exp_avg_sq": torch.from_numpy((0.01 * rng.standard_normal(p.shape) ** 2).astype(np.float32))}
    return ps, opt


def test_optimizer_state_with_group_steps_round_trips():
    """Group steps (0, 0, 3, 3) -- the front end never stepped -- through adam_state_dict / flatten_optimizer_state, and into a torch.optim.Adam whose
    next step equals the next step of the optimizer the state was taken from."""
    geo = D.geo_of("n32")
    shapes = [tuple(v.shape) for v in (O.init_params(geo, 4)[k] for k in O.param_order())]
    ps, opt = _adam_with_state(shapes, (0, 0, 3, 3), seed=2)
    flat = misc.flatten_optimizer_state(opt.state_dict(), shapes)
    assert flat is not None and flat["step"] == 3
    assert flat["steps"] == [0] * 4 + [3] * 36
    assert all(not flat["exp_avg"][i].any() and not flat["exp_avg_sq"][i].any() for i in range(4))
    osd = misc.adam_state_dict(flat["steps"], flat["lr"], [torch.from_numpy(a.reshape(s).copy()) for a, s in zip(flat["exp_avg"], shapes)],
                               [torch.from_numpy(a.reshape(s).copy()) for a, s in zip(flat["exp_avg_sq"], shapes)])
    assert [float(osd["state"][i]["step"]) for i in (0, 3, 4, 39)] == [0.0, 0.0, 3.0, 3.0]
    again = misc.flatten_optimizer_state(osd, shapes)
    assert again["steps"] == flat["steps"] and all(np.array_equal(a, b) for a, b in zip(again["exp_avg"] + again["exp_avg_sq"], flat["exp_avg"] + flat["exp_avg_sq"]))
    # one further step, everything trainable: the loaded optimizer against the original
    ps2 = [p.detach().clone().requires_grad_(True) for p in ps]
    opt2 = torch.optim.Adam(ps2, lr=1e-3)
    opt2.load_state_dict(osd)
    rng = np.random.default_rng(9)
    for p, q in zip(ps, ps2):
        g = torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32))
        p.grad, q.grad = g.clone(), g.clone()
    opt.step(); opt2.step()
    for i, (p, q) in enumerate(zip(ps, ps2)):
        assert torch.equal(p.detach(), q.detach()), i
    assert [int(opt2.state[ps2[i]]["step"]) for i in (0, 4)] == [1, 4]
    # steps that differ INSIDE a group: refused as before
    bad = opt.state_dict(); bad["state"][5]["step"] = torch.tensor(7.0)
    assert misc.flatten_optimizer_state(bad, shapes) is None


def test_equal_steps_keep_the_single_step_key():
    geo = D.geo_of("n32")
    shapes = [tuple(v.shape) for v in (O.init_params(geo, 4)[k] for k in O.param_order())]
    ps, opt = _adam_with_state(shapes, (5, 5, 5, 5), seed=3)
    flat = misc.flatten_optimizer_state(opt.state_dict(), shapes)
    assert flat["step"] == 5 and flat["steps"] == [5] * 40
    osd = misc.adam_state_dict(flat["step"], flat["lr"], [p.detach() for p in ps], [p.detach() for p in ps])      # the scalar form every caller used so far
    assert all(float(osd["state"][i]["step"]) == 5.0 for i in range(40))


def _stub_engine():
    from signaltrain_amd.engine import StepEngine
    eng = object.__new__(StepEngine)          # sync_trainable reads the model's flags and nothing of the device state
    eng.trainable = 15
    return eng


def _model():
    from signaltrain_amd import nn_proc
    nn_proc._QUIET = True
    return nn_proc.st_model(scale_factor=1, shrink_factor=4, num_knobs=4)


def test_sync_trainable_masks_and_refusals():
    from signaltrain_amd import nn_proc
    model, eng = _model(), _stub_engine()
    assert eng.sync_trainable(model) == 15
    nn_proc.freeze_layers([model.mpaec.dft_analysis, model.mpaec.dft_synthesis])
    assert all(not p.requires_grad for p in model.mpaec.dft_analysis.parameters())
    assert eng.sync_trainable(model) == 12 and eng.trainable == 12
    nn_proc.unfreeze_layers([model.mpaec.dft_synthesis]); nn_proc.freeze_layers([model.mpaec.aenc])
    assert eng.sync_trainable(model) == 2 | 8
    nn_proc.unfreeze_layers([model.mpaec])
    assert eng.sync_trainable(model) == 15
    model.mpaec.aenc.fnn_dec.bias.requires_grad = False                       # a mixed group
    with pytest.raises(ValueError, match="mpaec.aenc.fnn_dec.bias"):
        eng.sync_trainable(model)
    assert eng.trainable == 15                                                # ... left the mask as it was
    nn_proc.freeze_layers([model.mpaec])
    with pytest.raises(ValueError, match="nothing to train"):
        eng.sync_trainable(model)
    model.unfreeze(); nn_proc.unfreeze_layers([model.mpaec])
    model.freeze()                                                            # the pair the reference left commented out
    assert eng.sync_trainable(model) == 12
    model.unfreeze()
    assert eng.sync_trainable(model) == 15


def test_group_names_and_set_trainable():
    from signaltrain_amd.engine import StepEngine
    assert StepEngine.group_mask(("frontend",)) == 3 and StepEngine.group_mask(["aenc", "phs_aenc"]) == 12 and StepEngine.group_mask(14) == 14
    eng = _stub_engine()
    assert eng.set_trainable(("analysis", "aenc")) == 5 and eng.trainable == 5
    with pytest.raises(ValueError):
        eng.set_trainable(0)
    with pytest.raises(ValueError):
        eng.set_trainable(("encoder",))
    with pytest.raises(ValueError):
        eng.set_trainable(16)


def test_train_refuses_an_unknown_group_name():
    from signaltrain_amd import train
    with pytest.raises(ValueError, match="decoder"):
        train.train(freeze=("frontend", "decoder"), epochs=1, n_data_points=8, batch_size=4)
    with pytest.raises(ValueError, match="unfreeze_epoch"):
        train.train(unfreeze_epoch=1, epochs=2, n_data_points=8, batch_size=4)
