"""The oracle's rule for a train step with frozen parameter groups (st_train_step_groups), shared by tests/test_frozen_groups_host.py (which pins it
to torch's behaviour for requires_grad = False parameters under clip_grad_norm_ + torch.optim.Adam) and tests/test_gpu_frozen_groups.py (which pins the
device step to it).  Importing this needs no GPU.

The rule: gradients as oracle.st_oracle.model_loss_bwd gives them; the L1 clip of clip_l1_stft over the TRAINABLE tensors of the clip scope only (none:
norm 0, coefficient 1); adam_step on each trainable group with that group's own step number; a frozen group's parameters and moments are not touched."""
import numpy as np

from oracle import st_oracle as O

GROUP_BITS = (1, 2, 4, 8)                                        # ST_GROUP_ANALYSIS, _SYNTHESIS, _AE_MAG, _AE_PHS
GROUP_SLICES = (slice(0, 2), slice(2, 4), slice(4, 22), slice(22, 40))


def group_keys():
    order = O.param_order()
    assert len(order) == 40 and tuple(order[:4]) == tuple(O.STFT_KEYS)
    return [order[sl] for sl in GROUP_SLICES]


def stages_of(mask):
    """The stage rule of include/signaltrain_hip.h, written out: SYN_DGRAD 1, SYN_WGRAD 2, AE_BWD 4, AE_DINPUT 8, ANA_WGRAD 16."""
    s = 0
    if mask & 2:
        s |= 2
    if mask & (4 | 8 | 1):
        s |= 4 | 1
    if mask & 1:
        s |= 8 | 16
    return s


def apply_step(P, M, V, G, mask, steps, lr, clip_all=False, unscale=1.0):
    """One clip + Adam step of the rule on the dicts P, M, V (updated in place, float32 like O.adam_step leaves them) from the gradients G.  steps: the
    Adam step number of each group (read for the trainable ones).  Returns (norm, coefficient)."""
    keys = group_keys()
    G = {k: (g * g.dtype.type(unscale) if unscale != 1.0 else g) for k, g in G.items()}
    scope = [k for g, ks in enumerate(keys) if (mask & GROUP_BITS[g]) and (g < 2 or clip_all) for k in ks]
    sub = {k: G[k] for k in scope}
    norm, coef = O.clip_l1_stft(sub, all_params=True) if sub else (0.0, 1.0)      # all_params: "every key of the dict handed over"
    G.update(sub)
    for g, ks in enumerate(keys):
        if mask & GROUP_BITS[g]:
            Pg, Mg, Vg = ({k: D[k] for k in ks} for D in (P, M, V))
            O.adam_step(Pg, {k: G[k] for k in ks}, Mg, Vg, int(steps[g]), lr)
            for D, Dg in ((P, Pg), (M, Mg), (V, Vg)):
                D.update(Dg)
    return norm, coef
