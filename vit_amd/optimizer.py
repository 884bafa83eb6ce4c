"""Optimizer factory of the hot path: mirrors `OptModule` (reference src/opt/optimizer.py:1-173).

Same config keys, same scheduler table, same Lightning-style return value ({optimizer, lr_scheduler{scheduler, monitor,
...}}).  For a `MyViT` on an MI355X the three types the reference documents (`opt.type` in configs/config.yaml: 'Adam',
'AdamW', 'SGD') resolve to a fused optimizer: one HIP kernel over the flat parameter buffer that applies the global-norm
clip coefficient, the update and the bf16 shadow refresh in a single pass -- `FusedAdamW` (torch.optim.AdamW; with
`adam_l2` torch.optim.Adam, whose weight decay is L2 in the gradient) and `FusedSGD` (torch.optim.SGD), each verified
against its torch class in tests/.  Any other optimizer type falls through to torch.optim exactly as in the reference
(src/opt/optimizer.py:14-26,108; it then works on the `.grad` views the model's backward produces).
One type beside the reference's: `lamb` -> `FusedLamb` (timm's Lamb; torch.optim has none, so there is nothing to fall
through to and the type is an error on any other model), verified against a float64 restatement in tests/test_lamb_gpu.py.
And `muon` -> `FusedMuon`: Muon on the encoder's weight matrices (a grouped MFMA kernel runs the Newton-Schulz products of all
matrices in one launch each), AdamW on everything else; verified against torch.optim.Muon and a float64 restatement in
tests/test_muon_gpu.py.  torch's own Muon refuses every parameter that is not 2-D, so this type, too, is an error on any other model.
"""
from __future__ import annotations

import fnmatch
import re
from typing import Optional

import torch

from . import functional as vf

__all__ = ["OptModule", "FusedOptimizer", "FusedAdamW", "FusedLamb", "FusedMuon", "FusedSGD", "build_param_groups", "muon_matrix_names"]


class FusedOptimizer(torch.optim.Optimizer):
    """What the fused optimizers over MyViT's flat buffers share; a subclass adds its state buffers and its kernel.

    `step()` == the torch optimizer's: parameters without a gradient (frozen ones, the never-used pooler, everything when
    no backward ran) are left alone together with their state, exactly as torch skips them.  Parameters that are not slices
    of the engine's flat buffer (a trainable input preprocessor) are stepped by the same kernel on state buffers of their
    own, and their gradients join the global clipping norm.

    Gradient clipping: either the caller clips `.grad` beforehand (Lightning's gradient_clip_val path; the grads are
    views of the flat buffer, so that is seen here), or `set_grad_clip(max_norm)` fuses clip_grad_norm_(max_norm) into the
    step (norm kernel + coefficient applied on the fly).

    Under data parallelism (`attach_reducer`) the flat gradient buffer holds the rank-averaged gradient when `step()` runs;
    a `.grad` that is NOT the flat-buffer view (a hook or an accumulation replaced it) would silently overwrite that
    average with a local gradient, so it is an error there.  With a sharding reducer ('zero1') each rank updates only its
    shard of every sharded bucket and the updated parameters are all-gathered.

    Parameter groups (`param_groups=[{"params": [parameters or their names], "lr": ..., "weight_decay": ...}, ...]` at
    construction, or `add_param_group`; keys a group omits take the defaults; a parameter no group names is not stepped, as in
    torch).  One group or many, every active run of the flat buffer is ONE launch of the `*_step_groups` kernels
    (include/vit_amd_optim.h): they look each element's lr / weight_decay / momentum up in a segment table built from the
    partition (rebuilt when it changes) and a group table that is rewritten, ahead of the step, only when a scheduler changed a
    number; a single group is a table of one segment and one row.  The step captured as a hipGraph (vit_amd/graph.py) issues
    the same launch in its `dyn` form.  What the kernel shares across groups (`_SHARED`) must agree, else ValueError.

    A subclass provides: `_STATE` (attribute names of its flat state buffers, each None until allocated), `_SHARED`,
    `_ensure_state()`, `_group_values(group)` (the group's table row, validated), `_launch(lo, hi, tables, shadow, sqnorm, dyn)`
    (the table launch over flat[lo:hi]), `_update_extra(p, group, sqnorm)` and `_extra_buffers(p)` (a parameter outside the flat
    buffer, by value); optionally `_graph_betas()` / `_graph_signature()` / `_graph_validate()`."""

    _STATE = ()
    _SHARED = ()

    def __init__(self, model, defaults, param_groups=None):
        self.model = model
        if param_groups is None:
            params = [p for p in model.parameters()]
        else:
            by_name = dict(model.named_parameters())
            params = []
            for grp in param_groups:
                grp = dict(grp)
                members = grp["params"]
                members = [members] if isinstance(members, (str, torch.Tensor)) else list(members)
                unknown = [m for m in members if isinstance(m, str) and m not in by_name]
                if unknown:
                    raise ValueError(f"param_groups names parameters the model does not have: {unknown}")
                grp["params"] = [by_name[m] if isinstance(m, str) else m for m in members]
                params.append(grp)
        super().__init__(params, defaults)
        self._part = None
        self._refresh_members()
        self._extra_state = {}
        self._step = 0
        self._clip: Optional[float] = None
        self._sq = None
        self._reducer = None
        self.last_grad_norm: Optional[torch.Tensor] = None

    def set_grad_clip(self, max_norm: Optional[float]):
        self._clip = max_norm

    def attach_reducer(self, reducer):
        self._reducer = reducer

    # ------------------------------------------------------------------ parameter groups
    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, "_part"):  # torch's constructor adds the initial groups through here, before ours has run
            self._refresh_members()

    def _partition_signature(self):
        return tuple(tuple(id(p) for p in grp["params"]) for grp in self.param_groups)

    def _refresh_members(self):
        """Which group owns which parameter, and which owned parameters lie outside the engine's flat buffer."""
        own = {id(p) for p in getattr(self.model, "_param_list", [])}
        self._members_of = self._partition_signature()
        self._group_index = {id(p): gi for gi, grp in enumerate(self.param_groups) for p in grp["params"]}
        self._extras = [p for grp in self.param_groups for p in grp["params"] if id(p) not in own]

    def _group_for(self, p):
        return self.param_groups[self._group_index[id(p)]]

    def _all_params(self):
        """Every group's parameters in torch's state_dict numbering (consecutive across the groups)."""
        return [p for grp in self.param_groups for p in grp["params"]]

    def _partition(self):
        """(signature, device, vf.GroupTables) of the current partition of the flat buffer into groups; rebuilt when a
        parameter changed its group (or the buffer its device).  The pad behind an entry belongs to the entry."""
        sig, flat = self._partition_signature(), self.model.engine.flat
        if self._part is None or self._part[0] != sig or self._part[1] != flat.device:
            self._refresh_members()
            lay, triples = self.model.engine.layout, []
            for name, p in zip(self.model._param_names, self.model._param_list):
                off, _ = lay.entries[name]
                if off < lay.n_trainable and id(p) in self._group_index:
                    triples.append((off, (lay.numel(name) + 7) // 8 * 8, self._group_index[id(p)], name))
            if not triples:
                raise ValueError("no parameter group owns a parameter of the model's flat buffer")
            triples.sort()
            self._part = (sig, flat.device, self._build_tables(triples, flat.device))
        return self._part

    def _build_tables(self, triples, device):
        """The device tables over (offset, padded numel, group, name), sorted by offset: neighbours of one group merge."""
        return vf.optim_group_tables([t[:3] for t in triples], len(self.param_groups), device)

    def _check_shared(self):
        """beta1 / beta2 / eps, or nesterov / dampening, are one kernel argument for the whole launch."""
        first = self.param_groups[0]
        for gi, grp in enumerate(self.param_groups[1:], 1):
            for key in self._SHARED:
                a, b = first[key], grp[key]
                if (tuple(a) != tuple(b)) if isinstance(a, (tuple, list)) else (a != b):
                    raise ValueError(f"{type(self).__name__}: param_groups[{gi}]['{key}'] = {b} differs from group 0's {a}; the "
                                     f"fused step shares {', '.join(self._SHARED)} across all groups")

    def _sync_group_table(self):
        """The device group table <- the groups' current numbers, launched only when one changed; returns the tables."""
        self._check_shared()
        tables = self._partition()[2]
        vf.optim_groups_write(tables, [self._group_values(grp) for grp in self.param_groups])
        return tables

    def _flat_states(self):
        """The allocated flat state buffers, in `_STATE` order (all of them or none)."""
        bufs = [getattr(self, name) for name in self._STATE]
        return [] if any(b is None for b in bufs) else bufs

    def _ensure_flat(self, names):
        """Zero-filled buffers like the engine's flat buffer for `names`; one that was loaded before the model moved to the
        GPU is carried over."""
        flat = self.model.engine.flat
        for name in names:
            cur = getattr(self, name)
            if cur is None or cur.device != flat.device:
                new = torch.zeros_like(flat)
                if cur is not None:
                    new.copy_(cur)
                setattr(self, name, new)

    def _ensure_sq(self):
        eng = self.model.engine
        eng._ensure_device_state()
        if self._sq is None or self._sq.device != eng.flat.device:
            self._sq = torch.zeros(1, dtype=torch.float32, device=eng.flat.device)

    def _active_ranges(self):
        """Contiguous [lo, hi) runs of the flat buffer whose parameters have a gradient this step; also folds a replaced
        `.grad` back into the flat gradient buffer (single process only)."""
        eng, lay = self.model.engine, self.model.engine.layout
        spans = []
        for name, p in zip(self.model._param_names, self.model._param_list):
            off, _ = lay.entries[name]
            if off >= lay.n_trainable or p.grad is None or id(p) not in self._group_index:
                continue
            gv = eng.g(name)
            if p.grad.data_ptr() != gv.data_ptr():
                if self._reducer is not None:
                    raise RuntimeError(f"{name}.grad is not the flat gradient buffer's view (a hook or an accumulation into "
                                       f"an existing .grad replaced it): under data parallelism that would overwrite the "
                                       f"rank-averaged gradient with a local one")
                gv.copy_(p.grad)
            # the alignment pad behind an entry belongs to it (zeros in every buffer, never read back)
            spans.append((off, off + (lay.numel(name) + 7) // 8 * 8))
        spans.sort()
        runs = []
        for a, b in spans:
            if runs and runs[-1][1] == a:
                runs[-1][1] = b
            else:
                runs.append([a, b])
        return [(a, b) for a, b in runs]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        eng = self.model.engine
        self._ensure_state()
        if self._members_of != self._partition_signature():  # a group's member list was edited in place
            self._refresh_members()
        runs = self._active_ranges()
        extras = [p for p in self._extras if p.grad is not None]
        if not runs and not extras:
            return loss  # nothing has a gradient: torch.optim would not touch anything either
        self._step += 1
        red = self._reducer if (self._reducer is not None and getattr(self._reducer, "mode", "") == "zero1") else None
        if red is not None:
            runs = self._shard_runs(runs, red)
        sq = None
        if self._clip is not None:
            sq = self._sq
            first = True
            for a, b in (runs if red is None else self._norm_runs_local):
                vf.grad_sqnorm(eng.grads[a:b], out=sq, accumulate=not first)
                first = False
            if first:
                sq.zero_()
            if red is not None:  # shard sums -> global; the all-reduced buckets are added once (identical on every rank)
                torch.distributed.all_reduce(sq)
                for a, b in self._norm_runs_shared:
                    vf.grad_sqnorm(eng.grads[a:b], out=sq, accumulate=True)
            for p in extras:
                vf.grad_sqnorm(p.grad.contiguous().view(-1), out=sq, accumulate=True)
            self.last_grad_norm = sq
        shadow = eng.shadow if eng.precision == "bf16" else None  # f32 mode has no bf16 copy to refresh
        tables = self._sync_group_table() if runs else None  # no run (all of the flat buffer frozen): no table to ask for
        for a, b in runs:  # one launch per run: the kernel looks the groups up from the run's offset `a`
            self._launch(a, b, tables, shadow, sq)
        if red is not None:
            red.all_gather_params(eng.flat)
            if shadow is not None:
                vf.cast_f32_bf16(eng.flat, shadow)
        eng.mark_shadow_fresh()  # the kernel rewrote flat AND shadow through raw pointers
        for p in extras:
            self._update_extra(p, self._group_for(p), sq)
        return loss

    def _shard_runs(self, runs, red):
        """Intersect the active runs with what this rank updates under 'zero1': its shard of every sharded bucket, the whole
        of every all-reduced bucket.  Also records which pieces enter the norm locally (shards) / as shared (the rest)."""
        own, local, shared = [], [], []
        for (lo, hi), sh in zip(red.buckets, red.sharded):
            a, b = red.shard(lo, hi) if sh else (lo, hi)
            for ra, rb in runs:
                x, y = max(a, ra), min(b, rb)
                if x < y:
                    own.append((x, y))
                    (local if sh else shared).append((x, y))
        self._norm_runs_local, self._norm_runs_shared = local, shared
        return own

    def zero_grad(self, set_to_none: bool = True):
        super().zero_grad(set_to_none=True)

    def gather_sharded_state(self):
        """Under the 'zero1' exchange a rank's state buffers are current only inside its own shard of every sharded bucket.
        A checkpoint is written by rank 0 and read back by EVERY rank, so before `state_dict()` the shards are all-gathered
        into every rank's buffers (a collective: all ranks must call this; a no-op for the all-reduce exchange and for a
        single process).  Without it the other ranks resumed with zero moments (first update ~3x lr)."""
        red = self._reducer
        if red is None or getattr(red, "mode", "") != "zero1" or self._step == 0:
            return
        for buf in self._flat_states():
            red.all_gather_params(buf)

    # ------------------------------------------------------------------ everything a step changes in here, for a caller that
    # takes real steps and then undoes them (Trainer._snapshot / _restore, the warm-up steps of a graph capture)
    def clone_state(self):
        return {"step": self._step,
                "flat": [None if getattr(self, n) is None else getattr(self, n).clone() for n in self._STATE],
                "extra_state": {k: tuple(t.clone() for t in bufs) for k, bufs in self._extra_state.items()},
                "extras": [p.detach().clone() for p in self._extras]}

    def restore_state(self, saved):
        """Buffers that existed at `clone_state()` are copied back IN PLACE (a captured graph holds their addresses); one
        that did not exist then is dropped again."""
        self._step = saved["step"]
        for name, old in zip(self._STATE, saved["flat"]):
            if old is None:
                setattr(self, name, None)
            else:
                getattr(self, name).copy_(old)
        self._extra_state = saved["extra_state"]
        with torch.no_grad():
            for p, q in zip(self._extras, saved["extras"]):
                p.copy_(q)

    # ------------------------------------------------------------------ the captured step (vit_amd/graph.py)
    def _graph_betas(self):
        """(beta1, beta2) for vit_step_advance's bias corrections."""
        return 0.0, 0.0

    def _graph_signature(self):
        """What of this optimizer's set-up is frozen into a capture; `_graph_validate` raises ValueError when a replay would
        no longer be the eager step.  Here: the partition into groups -- the capture holds the segment table's address."""
        return self._partition_signature()

    def _graph_validate(self, signature):
        if signature != FusedOptimizer._graph_signature(self):
            raise ValueError("the optimizer's parameter groups were repartitioned after the step was captured")

    # ------------------------------------------------------------------ torch.optim-format state
    def _param_slices(self):
        """(torch's state_dict index, offset, numel, shape) of every trainable parameter in the flat buffer a group owns."""
        lay = self.model.engine.layout
        index = {id(p): i for i, p in enumerate(self._all_params())}
        for name, p in zip(self.model._param_names, self.model._param_list):
            off, shape = lay.entries[name]
            if off < lay.n_trainable and id(p) in index:
                yield index[id(p)], off, lay.numel(name), shape

    def _groups_dict(self):
        groups, start = [], 0
        for grp in self.param_groups:
            d = {k: (list(v) if isinstance(v, tuple) else v) for k, v in grp.items() if k != "params"}
            d["params"] = list(range(start, start + len(grp["params"])))
            start += len(grp["params"])
            groups.append(d)
        return groups

    def _load_groups(self, sd):
        for grp, src in zip(self.param_groups, sd.get("param_groups", [])):
            for k, v in src.items():
                if k != "params":
                    grp[k] = tuple(v) if k == "betas" else v


class FusedAdamW(FusedOptimizer):
    """AdamW over MyViT's flat buffers (see FusedOptimizer).  `step()` == torch.optim.AdamW.step(); `adam_l2=True` makes it
    torch.optim.Adam.step(): `weight_decay` is then L2 in the (clipped) gradient instead of a decoupled decay.
    `state_dict()` / `load_state_dict()` speak torch.optim.AdamW's (= Adam's) format (per-parameter `step`, `exp_avg`,
    `exp_avg_sq`, indexed in `model.parameters()` order), so optimizer state moves between this class and the reference's
    torch optimizer through a Lightning checkpoint."""

    _STATE = ("_m", "_v")
    _SHARED = ("betas", "eps")

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, adam_l2: bool = False,
                 param_groups=None):
        super().__init__(model, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), param_groups)
        self.adam_l2 = bool(adam_l2)
        self._m = None
        self._v = None

    def _ensure_state(self):
        self._ensure_sq()
        self._ensure_flat(self._STATE)

    def _group_values(self, grp):
        return float(grp["lr"]), float(grp["weight_decay"]), 0.0

    def _launch(self, lo, hi, tables, shadow, sq, dyn=False):
        """The update of flat[lo:hi]; `dyn` (inside a capture): the bias corrections come from the bound record."""
        eng, g0 = self.model.engine, self.param_groups[0]
        vf.adamw_step_groups(eng.flat[lo:hi], eng.grads[lo:hi], self._m[lo:hi], self._v[lo:hi],
                             None if shadow is None else shadow[lo:hi], tables, base=lo, beta1=g0["betas"][0],
                             beta2=g0["betas"][1], eps=g0["eps"], step=self._step, sqnorm=sq, max_norm=float(self._clip or 0.0),
                             l2=self.adam_l2, dyn=dyn)

    def _update_extra(self, p, grp, sq):
        m, v = self._extra_buffers(p)
        (vf.adam_l2_step if self.adam_l2 else vf.adamw_step)(
            p.data.view(-1), p.grad.contiguous().view(-1), m, v, None, lr=float(grp["lr"]), beta1=grp["betas"][0],
            beta2=grp["betas"][1], eps=grp["eps"], weight_decay=grp["weight_decay"], step=self._step, sqnorm=sq,
            max_norm=float(self._clip or 0.0))

    def _extra_buffers(self, p):
        st = self._extra_state.get(id(p))
        if st is None or st[0].device != p.device:
            st = self._extra_state[id(p)] = (torch.zeros_like(p.data).view(-1), torch.zeros_like(p.data).view(-1))
        return st

    def _graph_betas(self):
        return tuple(self.param_groups[0]["betas"])

    # ------------------------------------------------------------------ torch.optim.AdamW-format state
    def state_dict(self):
        index = {id(p): i for i, p in enumerate(self._all_params())}
        state = {}
        if self._m is not None and self._step > 0:
            for i, off, n, shape in self._param_slices():
                state[i] = {"step": torch.tensor(float(self._step)),
                            "exp_avg": self._m[off:off + n].detach().cpu().clone().view(shape),
                            "exp_avg_sq": self._v[off:off + n].detach().cpu().clone().view(shape)}
            for p in self._extras:
                st = self._extra_state.get(id(p))
                if st is not None:
                    state[index[id(p)]] = {"step": torch.tensor(float(self._step)),
                                           "exp_avg": st[0].detach().cpu().clone().view(p.shape),
                                           "exp_avg_sq": st[1].detach().cpu().clone().view(p.shape)}
        return {"state": state, "param_groups": self._groups_dict()}

    def load_state_dict(self, sd):
        if "state" not in sd:  # round-1 layout: flat moment buffers
            self._step = int(sd["step"])
            if sd.get("m") is not None:
                self._m, self._v = sd["m"].detach().clone().float(), sd["v"].detach().clone().float()
            for grp, src in zip(self.param_groups, sd.get("param_groups", [])):
                grp.update({k: v for k, v in src.items() if k != "params"})
            return
        lay = self.model.engine.layout
        flat = self.model.engine.flat
        if self._m is None or self._m.device != flat.device:
            self._m, self._v = torch.zeros_like(flat), torch.zeros_like(flat)
        params = self._all_params()
        names = {id(p): n for n, p in zip(self.model._param_names, self.model._param_list)}
        step = 0
        for idx, st in sd["state"].items():
            p = params[int(idx)]
            step = max(step, int(float(st["step"])))
            if id(p) in names:
                off, _ = lay.entries[names[id(p)]]
                n = lay.numel(names[id(p)])
                self._m[off:off + n].copy_(st["exp_avg"].reshape(-1))
                self._v[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
            else:
                self._extra_state[id(p)] = (st["exp_avg"].detach().clone().to(p.device).float().view(-1),
                                            st["exp_avg_sq"].detach().clone().to(p.device).float().view(-1))
        self._step = step
        self._load_groups(sd)


class FusedLamb(FusedAdamW):
    """LAMB over MyViT's flat buffers (see FusedOptimizer): timm's `Lamb`, the optimizer DeiT-III trains ViT-B with at a global
    batch of 2048, with the fused clip (`set_grad_clip`) in the place of timm's `max_grad_norm`; the formulas stand in
    include/vit_amd_optim.h.  Adam's moments, then per parameter tensor the trust ratio r = ||p|| / ||u|| scales the update
    (r = 1 for a tensor whose group has weight_decay 0 unless `always_adapt`; `trust_clip`: min(r, 1)).  The norms are per
    TENSOR, so the segment table has one segment per parameter (vf.optim_param_tables), not FusedAdamW's merged runs.
    `state_dict()` / `load_state_dict()` are FusedAdamW's (torch.optim.AdamW's format: LAMB keeps the same two moments), so a
    FusedAdamW checkpoint loads and `Trainer`'s exact resume works unchanged.
    `last_trust_ratios`: (names, ratios) of the last step -- `ratios` the device tensor the kernels wrote, one f32 per entry of
    `names` (the parameters in table order); None before the first step.  Entries of tensors the last step did not update
    (frozen ones) keep their previous value (1 initially).
    Under the 'zero1' exchange a rank's shard cuts tensors and a per-tensor norm would need a collective: not supported
    (`attach_reducer` raises ValueError); the all-reduce exchange needs nothing, every rank computes the same ratios."""

    _SHARED = ("betas", "eps", "always_adapt", "trust_clip")

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, always_adapt: bool = False,
                 trust_clip: bool = False, param_groups=None):
        FusedOptimizer.__init__(self, model, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                                  always_adapt=bool(always_adapt), trust_clip=bool(trust_clip)), param_groups)
        self.adam_l2 = False
        self._m = None
        self._v = None
        self._trust = None        # one f32 per segment of the table, written by the kernels
        self._trust_extra = {}    # id(p) -> one f32, for a parameter outside the flat buffer
        self._stepped = False

    def attach_reducer(self, reducer):
        if getattr(reducer, "mode", "") == "zero1":
            raise ValueError("FusedLamb does not support the 'zero1' exchange: its shards cut parameter tensors and a trust "
                             "ratio is a norm over a whole tensor; use the all-reduce exchange")
        super().attach_reducer(reducer)

    def _build_tables(self, triples, device):
        """One segment per parameter tensor, and a trust entry per segment (1 until a step writes it)."""
        tables = vf.optim_param_tables([t[:3] for t in triples], len(self.param_groups), device)
        self._trust_names = [t[3] for t in triples]
        self._trust_index = torch.tensor(tables.segment_of, dtype=torch.long, device=device)
        self._trust = torch.ones(tables.n_segments, dtype=torch.float32, device=device)
        return tables

    def _launch(self, lo, hi, tables, shadow, sq, dyn=False):
        eng, g0 = self.model.engine, self.param_groups[0]
        self._stepped = True
        vf.lamb_step_groups(eng.flat[lo:hi], eng.grads[lo:hi], self._m[lo:hi], self._v[lo:hi],
                            None if shadow is None else shadow[lo:hi], tables, self._trust, base=lo, beta1=g0["betas"][0],
                            beta2=g0["betas"][1], eps=g0["eps"], always_adapt=g0["always_adapt"], trust_clip=g0["trust_clip"],
                            step=self._step, sqnorm=sq, max_norm=float(self._clip or 0.0), dyn=dyn)

    def _update_extra(self, p, grp, sq):
        m, v = self._extra_buffers(p)
        trust = self._trust_extra.get(id(p))
        if trust is None or trust.device != p.device:
            trust = self._trust_extra[id(p)] = torch.ones(1, dtype=torch.float32, device=p.device)
        self._stepped = True
        vf.lamb_step(p.data.view(-1), p.grad.contiguous().view(-1), m, v, None, lr=float(grp["lr"]), beta1=grp["betas"][0],
                     beta2=grp["betas"][1], eps=grp["eps"], weight_decay=grp["weight_decay"], always_adapt=grp["always_adapt"],
                     trust_clip=grp["trust_clip"], step=self._step, sqnorm=sq, max_norm=float(self._clip or 0.0), trust=trust)

    @property
    def last_trust_ratios(self):
        """(names, ratios): the last step's trust ratio of every parameter a group owns, the flat buffer's in table order, then
        the parameters outside it; `ratios` is a device tensor (reading it synchronises).  None before the first step."""
        if not self._stepped:
            return None
        names, parts = [], []
        if self._trust is not None:
            names += self._trust_names
            parts.append(self._trust[self._trust_index])
        by_id = {id(p): n for n, p in self.model.named_parameters()}
        for p in self._extras:
            if id(p) in self._trust_extra:
                names.append(by_id.get(id(p), "?"))
                parts.append(self._trust_extra[id(p)])
        return names, torch.cat(parts)


MUON_STEMS = ("attention.attention.query", "attention.attention.key", "attention.attention.value", "attention.output.dense",
              "intermediate.dense", "output.dense")
_MUON_NAME = re.compile(r"^vit\.encoder\.layer\.\d+\.(?:" + "|".join(re.escape(s) for s in MUON_STEMS) + r")\.weight$")
_MUON_KEYS = ("momentum", "nesterov", "ns_steps", "ns_coefficients", "eps", "adjust_lr")


def muon_matrix_names(names):
    """Of `names`, the Muon matrices: the six 2-D weights of every encoder layer (query, key and value each on its own, as
    torch.optim.Muon would be given them).  Everything else -- biases, LayerNorms, tokens, positions, LayerScale, the patch
    projection, the head, a decoder -- steps with AdamW."""
    return [n for n in names if _MUON_NAME.match(n)]


class _MuonRun:
    """What one `_launch(lo, hi)` of FusedMuon issues: the AdamW sub-runs around the matrices, and the matrices' tables, plan
    and per-matrix scale cells (None when the run holds no trainable matrix)."""

    def __init__(self, adam_runs, names, tables, plan, part, inv_norm, norms):
        self.adam_runs, self.names, self.tables, self.plan = adam_runs, names, tables, plan
        self.part, self.inv_norm, self.norms = part, inv_norm, norms


class FusedMuon(FusedAdamW):
    """Muon on the encoder's weight matrices, AdamW on everything else, in one optimizer over MyViT's flat buffers (see
    FusedOptimizer; the formulas stand in include/vit_amd_muon.h).  For each of `muon_matrix_names`: SGD momentum in an f32 buffer,
    its Newton-Schulz orthogonalisation in bf16 (torch.optim.Muon's rounding points), and W = W (1 - lr wd) - lr ratio O with the
    group's lr / weight_decay and ratio = torch's `_adjust_lr` (`adjust_lr`: 'match_rms_adamw' -- the default, so that one lr and
    one weight_decay serve both halves --, 'original', 'none').  Every other tensor takes FusedAdamW's launch over the sub-runs
    between the matrices, bit for bit FusedAdamW's result.  A frozen matrix is neither read nor written, nor is its buffer.
    A step is, per active run: one vit_adamw_step_groups launch per sub-run between matrices (4 per encoder layer and the
    embeddings': 49 at ViT-B), then 4 + 3 * ns_steps launches for all of the run's matrices together.
    `state_dict()` holds torch.optim.Muon's {"momentum_buffer"} for a matrix and AdamW's {"step", "exp_avg", "exp_avg_sq"} for
    the rest.  `last_ns_norms`: (names, norms) of the last step's ||X0||_F per matrix, a device tensor; None before a step.
    The 'zero1' exchange is refused for LAMB's reason: a shard cuts matrices."""

    _STATE = ("_m", "_v", "_buf")
    _SHARED = ("betas", "eps", "momentum", "nesterov", "ns_steps", "ns_coefficients", "muon_eps", "adjust_lr")

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, momentum=0.95, nesterov=True, ns_steps=5,
                 ns_coefficients=(3.4445, -4.775, 2.0315), muon_eps=1e-7, adjust_lr="match_rms_adamw", param_groups=None):
        if not 0.0 <= float(momentum) < 1.0:
            raise ValueError(f"FusedMuon: momentum = {momentum} must lie in [0, 1)")
        if int(ns_steps) != ns_steps or not 0 <= int(ns_steps) < 100:
            raise ValueError(f"FusedMuon: ns_steps = {ns_steps} must be an integer in [0, 100)")
        if len(tuple(ns_coefficients)) != 3:
            raise ValueError(f"FusedMuon: ns_coefficients = {ns_coefficients} must be three numbers (a, b, c)")
        if not float(muon_eps) > 0:
            raise ValueError(f"FusedMuon: eps = {muon_eps} must be positive")
        vf.muon_adjust_ratio(adjust_lr, 16, 16)  # ValueError on an unknown mode
        FusedOptimizer.__init__(self, model, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, momentum=float(momentum),
                                                  nesterov=bool(nesterov), ns_steps=int(ns_steps),
                                                  ns_coefficients=tuple(float(c) for c in ns_coefficients),
                                                  muon_eps=float(muon_eps), adjust_lr=adjust_lr or "none"), param_groups)
        self.adam_l2 = False
        self._m = None
        self._v = None
        self._buf = None     # f32, compact: the matrices one behind the other (MuonTables' xoff)
        self._x = None       # the two bf16 X workspaces, compact like _buf
        self._mats = None    # [(name, parameter, off, xoff, rows, cols)] of every Muon matrix a group owns, by offset
        self._runs = {}
        self._last_runs, self._last_step = [], -1

    def attach_reducer(self, reducer):
        if getattr(reducer, "mode", "") == "zero1":
            raise ValueError("FusedMuon does not support the 'zero1' exchange: its shards cut weight matrices and the "
                             "orthogonalisation is a function of a whole matrix; use the all-reduce exchange")
        super().attach_reducer(reducer)

    # ------------------------------------------------------------------ the split
    def _matrices(self):
        if self._mats is None:
            lay, by_name = self.model.engine.layout, dict(zip(self.model._param_names, self.model._param_list))
            mats, xoff = [], 0
            for name in sorted(muon_matrix_names(self.model._param_names), key=lambda n: lay.entries[n][0]):
                off, (rows, cols) = lay.entries[name]
                if off < lay.n_trainable and id(by_name[name]) in self._group_index:
                    mats.append((name, by_name[name], off, xoff, rows, cols))
                xoff += rows * cols  # a matrix's place in the compact buffers does not depend on who owns its neighbours
            self._mats, self._mat_total = mats, xoff
        return self._mats

    def muon_split(self):
        """(names of the Muon matrices, names of the AdamW-side tensors) among the flat buffer's trainable parameters a group owns."""
        lay, mats = self.model.engine.layout, {m[0] for m in self._matrices()}
        owned = [n for n, p in zip(self.model._param_names, self.model._param_list)
                 if lay.entries[n][0] < lay.n_trainable and id(p) in self._group_index]
        return [n for n in owned if n in mats], [n for n in owned if n not in mats]

    def _refresh_members(self):
        super()._refresh_members()
        self._mats, self._runs = None, {}

    def _ensure_state(self):
        self._ensure_sq()
        self._ensure_flat(("_m", "_v"))
        self._matrices()
        dev = self.model.engine.flat.device
        if self._buf is None or self._buf.device != dev:
            new = torch.zeros(max(self._mat_total, 8), dtype=torch.float32, device=dev)
            if self._buf is not None:
                new.copy_(self._buf)
            self._buf, self._runs = new, {}
        if self._x is None or self._x[0].device != dev:
            self._x = [torch.zeros(max(self._mat_total, 8), dtype=torch.bfloat16, device=dev) for _ in range(2)]
            self._runs = {}

    def _run_for(self, lo, hi):
        """The `_MuonRun` of flat[lo:hi]: cached per run, partition and set of frozen matrices."""
        mats = [m for m in self._matrices() if m[2] < hi and m[2] + m[4] * m[5] > lo]
        key = (lo, hi, self._partition_signature(), tuple(m[1].requires_grad for m in mats))
        run = self._runs.get(key)
        if run is None:
            g0, dev = self.param_groups[0], self.model.engine.flat.device
            vf.muon_check_run([(m[2], m[4], m[5]) for m in mats], lo, hi - lo)  # ValueError: the run cuts a matrix
            adam_runs, at = [], lo
            for _, _, off, _, rows, cols in mats:
                if off > at:
                    adam_runs.append((at, off))
                at = off + rows * cols
            if at < hi:
                adam_runs.append((at, hi))
            live = [m for m in mats if m[1].requires_grad]
            if live:
                tables = vf.muon_mat_table([(off, xoff, rows, cols, self._group_index[id(p)],
                                             vf.muon_adjust_ratio(g0["adjust_lr"], rows, cols))
                                            for _, p, off, xoff, rows, cols in live], dev, total=self.model.engine.flat.numel(),
                                           compact_total=self._buf.numel())
                run = _MuonRun(adam_runs, [m[0] for m in live], tables, vf.MuonPlan(tables, g0["ns_coefficients"], dev, x=self._x),
                               torch.zeros(tables.n_tiles, dtype=torch.float64, device=dev),
                               torch.zeros(tables.n_mats, dtype=torch.float32, device=dev),
                               torch.zeros(tables.n_mats, dtype=torch.float32, device=dev))
            else:
                run = _MuonRun(adam_runs, [], None, None, None, None, None)
            self._runs[key] = run
        return run

    def _launch(self, lo, hi, tables, shadow, sq, dyn=False):
        eng, g0 = self.model.engine, self.param_groups[0]
        run = self._run_for(lo, hi)
        for a, b in run.adam_runs:
            FusedAdamW._launch(self, a, b, tables, shadow, sq, dyn=dyn)
        if self._last_step != self._step:
            self._last_runs, self._last_step = [], self._step
        if run.tables is None:
            return
        if run not in self._last_runs:
            self._last_runs.append(run)
        vf.muon_momentum(eng.grads, self._buf, self._x[1], run.tables, run.part, momentum=g0["momentum"], nesterov=g0["nesterov"],
                         sqnorm=sq, max_norm=float(self._clip or 0.0))
        vf.muon_norms(run.tables, run.part, run.inv_norm, run.norms, eps=g0["muon_eps"])
        vf.muon_normalize(self._x[1], self._x[0], run.tables, run.inv_norm)
        out = run.plan.iterate(g0["ns_steps"], start=0)
        vf.muon_apply(eng.flat, shadow, out, run.tables, tables.groups)

    @property
    def last_ns_norms(self):
        """(names, norms): ||X0||_F of every matrix the last step orthogonalised, in flat-buffer order; `norms` is a device tensor
        (reading it synchronises).  None before the first step."""
        if not self._last_runs:
            return None
        return [n for r in self._last_runs for n in r.names], torch.cat([r.norms for r in self._last_runs])

    def _graph_signature(self):
        return super()._graph_signature(), tuple(m[1].requires_grad for m in self._matrices())

    def _graph_validate(self, signature):
        partition, frozen = signature
        super()._graph_validate(partition)
        if frozen != tuple(m[1].requires_grad for m in self._matrices()):
            raise ValueError("a Muon matrix was frozen or released after the step was captured")

    # ------------------------------------------------------------------ state: torch.optim.Muon's for a matrix, AdamW's for the rest
    def state_dict(self):
        sd = super().state_dict()
        if self._buf is not None and self._step > 0:
            index = {id(p): i for i, p in enumerate(self._all_params())}
            for _, p, _, xoff, rows, cols in self._matrices():
                sd["state"][index[id(p)]] = {
                    "momentum_buffer": self._buf[xoff:xoff + rows * cols].detach().cpu().clone().view(rows, cols)}
        return sd

    def load_state_dict(self, sd):
        if "state" not in sd:  # FusedAdamW's round-1 layout (flat moment buffers): no momentum buffers in it
            return super().load_state_dict(sd)
        params = self._all_params()
        mats = {id(m[1]): m for m in self._matrices()}
        dev, size = self.model.engine.flat.device, max(self._mat_total, 8)
        if self._buf is not None and self._buf.device == dev and self._buf.numel() == size:
            self._buf.zero_()  # in place: a captured step holds the buffer's address (and the cached runs stay valid)
        else:
            self._buf, self._runs = torch.zeros(size, dtype=torch.float32, device=dev), {}
        rest = {}
        for idx, st in sd["state"].items():
            m = mats.get(id(params[int(idx)]))
            if m is not None and "momentum_buffer" in st:
                self._buf[m[3]:m[3] + m[4] * m[5]].copy_(st["momentum_buffer"].reshape(-1))
            elif m is None:
                rest[idx] = st
        super().load_state_dict({"state": rest, "param_groups": sd.get("param_groups", [])})
        for grp in self.param_groups:
            grp["ns_coefficients"] = tuple(grp["ns_coefficients"])


class FusedSGD(FusedOptimizer):
    """SGD over MyViT's flat buffers (see FusedOptimizer).  `step()` == torch.optim.SGD.step() with dampening 0.
    `param_groups[0]` carries torch SGD's keys, and `lr` and `momentum` are read from it on every step: a one-cycle scheduler
    cycles both (it raises SGD's momentum from the reference's 0 to 0.85 .. 0.95).  The flat momentum buffer (and one per
    parameter outside the flat buffer) is allocated, as zeros, by the first step that sees momentum != 0: with dampening 0 a
    zero buffer gives exactly torch's first step (buf = g'), also for a parameter that is unfrozen mid-run.
    `state_dict()` / `load_state_dict()` speak torch.optim.SGD's format (per-parameter `momentum_buffer`, indexed in
    `model.parameters()` order, absent while no buffer exists)."""

    _STATE = ("_buf",)
    _SHARED = ("nesterov", "dampening")

    def __init__(self, model, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, param_groups=None):
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=False, foreach=None, differentiable=False, fused=None)
        self._group_values(defaults)
        super().__init__(model, defaults, param_groups)
        self._buf = None

    def _ensure_state(self):
        self._ensure_sq()
        if self._buf is not None or any(grp["momentum"] != 0 for grp in self.param_groups):
            self._ensure_flat(self._STATE)

    def _group_values(self, grp):
        """The group's table row; what FusedSGD refuses is refused here, for the constructor's defaults and on every step."""
        if grp["dampening"] != 0 or grp.get("maximize"):
            raise ValueError("FusedSGD supports neither dampening nor maximize (dampening = 0: a zero momentum buffer then "
                             "reproduces torch's first step)")
        lr, wd, mu = float(grp["lr"]), float(grp["weight_decay"]), float(grp["momentum"])
        if lr < 0 or mu < 0 or wd < 0:
            raise ValueError(f"FusedSGD: lr = {lr}, momentum = {mu}, weight_decay = {wd} must not be negative")
        if grp["nesterov"] and mu <= 0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        return lr, wd, mu

    def _launch(self, lo, hi, tables, shadow, sq, dyn=False):
        """The update of flat[lo:hi]; whether there is a momentum buffer at all, and nesterov, are frozen into a capture."""
        eng = self.model.engine
        vf.sgd_step_groups(eng.flat[lo:hi], eng.grads[lo:hi], None if self._buf is None else self._buf[lo:hi],
                           None if shadow is None else shadow[lo:hi], tables, base=lo,
                           nesterov=bool(self.param_groups[0]["nesterov"]), sqnorm=sq, max_norm=float(self._clip or 0.0), dyn=dyn)

    def _update_extra(self, p, grp, sq):
        lr, wd, mu = self._group_values(grp)
        vf.sgd_step(p.data.view(-1), p.grad.contiguous().view(-1), *(self._extra_buffers(p) or (None,)), None, lr=lr, momentum=mu,
                    weight_decay=wd, nesterov=bool(grp["nesterov"]), sqnorm=sq, max_norm=float(self._clip or 0.0))

    def _extra_buffers(self, p):
        if self._group_for(p)["momentum"] == 0:
            return ()
        st = self._extra_state.get(id(p))
        if st is None or st[0].device != p.device:
            st = self._extra_state[id(p)] = (torch.zeros_like(p.data).view(-1),)
        return st

    def _graph_signature(self):
        return self._buf is not None, super()._graph_signature()

    def _graph_validate(self, signature):
        had_buffer, partition = signature
        super()._graph_validate(partition)
        mu = max(grp["momentum"] for grp in self.param_groups)
        if mu != 0 and not had_buffer:  # (a momentum that becomes 0 needs nothing: the kernel skips such a row's buffer itself)
            raise ValueError(f"SGD's momentum became {mu} after the step was captured without a momentum buffer")

    # ------------------------------------------------------------------ torch.optim.SGD-format state
    def state_dict(self):
        index = {id(p): i for i, p in enumerate(self._all_params())}
        state = {}
        if self._buf is not None:
            for i, off, n, shape in self._param_slices():
                state[i] = {"momentum_buffer": self._buf[off:off + n].detach().cpu().clone().view(shape)}
        for p in self._extras:
            st = self._extra_state.get(id(p))
            if st is not None:
                state[index[id(p)]] = {"momentum_buffer": st[0].detach().cpu().clone().view(p.shape)}
        return {"state": state, "param_groups": self._groups_dict()}

    def load_state_dict(self, sd):
        lay = self.model.engine.layout
        params = self._all_params()
        names = {id(p): n for n, p in zip(self.model._param_names, self.model._param_list)}
        self._buf, self._extra_state = None, {}
        for idx, st in sd["state"].items():
            buf = st.get("momentum_buffer")
            if buf is None:
                continue
            p = params[int(idx)]
            if id(p) in names:
                if self._buf is None:
                    self._buf = torch.zeros_like(self.model.engine.flat)
                off, _ = lay.entries[names[id(p)]]
                self._buf[off:off + lay.numel(names[id(p)])].copy_(buf.reshape(-1))
            else:
                self._extra_state[id(p)] = (buf.detach().clone().to(p.device).float().view(-1),)
        self._load_groups(sd)


# ---------------------------------------------------------------------------------------------------------------- factory
_OPTIMIZERS = {
    "adam": "Adam", "adamw": "AdamW", "sgd": "SGD", "rmsprop": "RMSprop", "adadelta": "Adadelta", "adagrad": "Adagrad",
    "adamax": "Adamax", "asgd": "ASGD", "lbfgs": "LBFGS", "rprop": "Rprop", "sparseadam": "SparseAdam",
}
_SCHEDULERS = {
    "cosine": "CosineAnnealingLR", "cosineannealing": "CosineAnnealingLR", "cosineannealinglr": "CosineAnnealingLR",
    "onecycle": "OneCycleLR", "constant": "ConstantLR", "constantlr": "ConstantLR", "plateau": "ReduceLROnPlateau",
}


def _family(name: str) -> str:
    """Which argument rules a scheduler name falls under (substring match, first hit wins, as the reference resolves it)."""
    for fam in ("cosine", "onecycle", "constant", "plateau"):
        if fam in name:
            return fam
    return ""


# per family: (required arguments as {kwarg: how to get it}, optional keys copied only when present in the config)
def _scheduler_kwargs(fam: str, cfg: dict, lr: float) -> dict:
    if fam == "cosine":
        kw = {"T_max": cfg.get("T_max", cfg.get("ep", 100))}
        optional = ("eta_min",)
    elif fam == "onecycle":  # the run length (steps_per_epoch, epochs) is injected by configure_optimizers
        kw = {"max_lr": lr}
        optional = ("steps_per_epoch", "epochs", "pct_start", "div_factor", "final_div_factor")
    elif fam == "constant":
        kw = {"factor": cfg.get("factor", 1.0), "total_iters": cfg.get("total_iters", 1)}
        optional = ()
    elif fam == "plateau":
        kw = {"factor": cfg.get("factor", 0.1), "patience": cfg.get("patience", 10)}
        optional = ("mode",)
    else:
        return {}
    kw.update({k: cfg[k] for k in optional if k in cfg})
    return kw


_NO_DECAY_NAMES = ("vit.embeddings.cls_token", "vit.embeddings.position_embeddings", "vit.embeddings.mask_token",  # mask_token: 'mim' models
                   "vit.embeddings.register_tokens")  # model.num_register_tokens > 0
_LAYER = re.compile(r"(?:^|\.)encoder\.layer\.(\d+)\.")


def _layer_id(name: str, n_layers: int) -> int:
    """Depth of a parameter for `opt.layer_decay`: 0 for the embeddings, i + 1 for encoder layer i, L + 1 for what follows the
    encoder (final LayerNorm, pooler, head) -- and for whatever sits outside the ViT's depth (an input preprocessor), which
    therefore keeps `lr`."""
    m = _LAYER.search(name)
    if m:
        return int(m.group(1)) + 1
    return 0 if name.startswith("vit.embeddings.") else n_layers + 1


def build_param_groups(model, lr: float, weight_decay, no_decay=None, layer_decay=None):
    """torch-style parameter groups over `model.named_parameters()` for `opt.no_decay` / `opt.layer_decay`, or None when
    neither is set.  Every parameter lands in exactly one group; groups are ordered by depth, the decaying one first.

    no_decay: True = weight_decay 0 for parameters of at most one dimension (biases, LayerNorm weight and bias) and for
    vit.embeddings.cls_token / vit.embeddings.position_embeddings (the Conv1D patch weight [D, 1, P] decays); a list = exactly
    the parameters whose name matches one of its fnmatch patterns.
    layer_decay f: lr * f ** (L + 1 - id), id as in `_layer_id`."""
    if not no_decay and layer_decay is None:
        return None
    named = list(model.named_parameters())
    if isinstance(no_decay, str):
        no_decay = [no_decay]
    n_layers = 1 + max((int(m.group(1)) for m in (_LAYER.search(n) for n, _ in named) if m), default=-1)
    groups = {}
    for name, p in named:
        if no_decay is True:
            skip = p.ndim <= 1 or name in _NO_DECAY_NAMES
        else:
            skip = bool(no_decay) and any(fnmatch.fnmatchcase(name, pat) for pat in no_decay)
        depth = n_layers + 1 if layer_decay is None else _layer_id(name, n_layers)
        groups.setdefault((depth, skip), []).append(p)
    scale = 1.0 if layer_decay is None else float(layer_decay)
    return [{"params": members, "lr": lr * scale ** (n_layers + 1 - depth), "weight_decay": 0.0 if skip else weight_decay}
            for (depth, skip), members in sorted(groups.items(), key=lambda kv: kv[0])]


class OptModule:
    """The optimizer / scheduler factory behind `configure_optimizers` (reference: src/opt/optimizer.py:1-173).  Same config
    keys (`lr`, `type`, `weight_decay`, `lr_sch`, `warmup.{ratio,epochs}` / `warmup_ratio` / `warmup_epochs`, the scheduler's
    own keys), same result shape (an optimizer, or Lightning's {"optimizer", "lr_scheduler": {scheduler, monitor, ...}});
    behaviour pinned case by case on the reference's class in tests/golden/opt.json.

    Two keys beside the reference's, both absent by default (then nothing differs): `no_decay` and `layer_decay`
    (`build_param_groups`).  With either, every optimizer type -- fused or torch's -- is built over those parameter groups, and
    a one-cycle scheduler gets the groups' rates as its `max_lr` list (a scalar would flatten them)."""

    def __init__(self, lr, monitor_metric="loss", opt_type="adam", weight_decay=0.0, lr_scheduler_name=None,
                 warmup_ratio=0.0, warmup_epochs=None, no_decay=None, layer_decay=None, lamb_options=None, muon_options=None,
                 **kwargs) -> None:
        self.lamb_options = dict(lamb_options or {})  # eps / always_adapt / trust_clip of `type: lamb`
        self.muon_options = dict(muon_options or {})  # the `opt.muon` section of `type: muon`
        unknown = sorted(set(self.muon_options) - set(_MUON_KEYS))
        if unknown:
            raise ValueError(f"opt.muon: unknown keys {unknown}; known: {list(_MUON_KEYS)}")
        self.no_decay = no_decay
        self.layer_decay = None if layer_decay is None else float(layer_decay)
        self.lr = float(lr)
        self.monitor_metric = monitor_metric
        self.opt_type = opt_type
        self.weight_decay = weight_decay
        self.lr_scheduler_name = lr_scheduler_name
        self.warmup_ratio = warmup_ratio
        self.warmup_epochs = warmup_epochs
        self.kwargs = kwargs
        self.opt_fns = {k: getattr(torch.optim, v) for k, v in _OPTIMIZERS.items()}
        self.lr_schedulers = {k: getattr(torch.optim.lr_scheduler, v) for k, v in _SCHEDULERS.items()}

    @classmethod
    def from_config(cls, config):
        lr = config.get("lr", 1e-3)
        warm = config.get("warmup", {})
        common = dict(
            lr=lr, monitor_metric=config.get("monitor_metric", "loss"), opt_type=config.get("type", "adam").lower(),
            weight_decay=config.get("weight_decay", 0),
            warmup_ratio=warm.get("ratio", config.get("warmup_ratio", 0.0)),
            warmup_epochs=warm.get("epochs", config.get("warmup_epochs", None)),
        )
        for key in ("no_decay", "layer_decay"):  # absent by default: the reference's call, argument for argument
            if config.get(key) is not None and config.get(key) is not False:
                common[key] = config[key]
        if common["opt_type"] == "lamb":  # read only for this type
            common["lamb_options"] = {k: config[k] for k in ("eps", "always_adapt", "trust_clip") if config.get(k) is not None}
        if common["opt_type"] == "muon":  # likewise: the `opt.muon` section
            common["muon_options"] = dict(config.get("muon") or {})
        if "lr_sch" not in config:
            return cls(**common)
        name = config["lr_sch"].lower()
        return cls(lr_scheduler_name=name, **common, **_scheduler_kwargs(_family(name), config, lr))

    def _make_optimizer(self, model):
        from .specvit import MyViT

        groups = build_param_groups(model, self.lr, self.weight_decay, self.no_decay, self.layer_decay)
        fused = {} if groups is None else {"param_groups": groups}
        if self.opt_type == "lamb":  # ahead of `opt_fns`, which stays the reference's table: torch.optim has no LAMB
            if not isinstance(model, MyViT):
                raise ValueError("opt.type 'lamb' is the fused LAMB over a MyViT's flat buffers (FusedLamb); torch has no LAMB "
                                 f"to fall through to for a {type(model).__name__}")
            return FusedLamb(model, lr=self.lr, weight_decay=self.weight_decay, **self.lamb_options, **fused)
        if self.opt_type == "muon":  # torch.optim.Muon refuses every parameter that is not 2-D: nothing to fall through to either
            if not isinstance(model, MyViT):
                raise ValueError("opt.type 'muon' is the fused Muon + AdamW hybrid over a MyViT's flat buffers (FusedMuon); "
                                 f"there is nothing to fall through to for a {type(model).__name__}")
            opts = {("muon_eps" if k == "eps" else k): v for k, v in self.muon_options.items()}
            return FusedMuon(model, lr=self.lr, weight_decay=self.weight_decay, **opts, **fused)
        if isinstance(model, MyViT) and self.opt_type in ("adam", "adamw"):
            # torch.optim.Adam's weight_decay is L2-in-the-gradient; with the reference's default weight_decay=0
            # (optimizer.py:51) Adam == AdamW, and only with a decay does 'adam' need the L2 form of the kernel
            return FusedAdamW(model, lr=self.lr, weight_decay=self.weight_decay,
                              adam_l2=self.opt_type == "adam" and bool(self.weight_decay), **fused)
        if isinstance(model, MyViT) and self.opt_type == "sgd":
            return FusedSGD(model, lr=self.lr, weight_decay=self.weight_decay, **fused)
        return self.opt_fns[self.opt_type](model.parameters() if groups is None else groups, lr=self.lr,
                                           weight_decay=self.weight_decay)

    def _warmup_length(self) -> Optional[int]:
        """Epochs of linear warm-up in front of the scheduler, or None.  One-cycle brings its own."""
        wanted = self.warmup_ratio > 0 or self.warmup_epochs is not None
        if not wanted or "onecycle" in self.lr_scheduler_name:
            return None
        if self.warmup_epochs is not None:
            return self.warmup_epochs
        horizon = self.kwargs.get("T_max", self.kwargs.get("epochs", 100))
        return max(1, int(horizon * self.warmup_ratio))

    def __call__(self, model):
        optimizer = self._make_optimizer(model)
        name = self.lr_scheduler_name
        if name is None:
            return optimizer
        if name not in self.lr_schedulers:
            raise ValueError(f"Unknown scheduler: {name}")
        sched_mod = torch.optim.lr_scheduler
        n_warm = self._warmup_length()
        kwargs = self.kwargs
        if len(optimizer.param_groups) > 1 and "max_lr" in kwargs:  # one-cycle: each group cycles up to its own rate
            kwargs = dict(kwargs, max_lr=[grp["lr"] for grp in optimizer.param_groups])
        if n_warm is None:
            scheduler = self.lr_schedulers[name](optimizer, **kwargs)
        else:  # LinearLR from 10 % of the target rate, then the scheduler proper (constructed in this order: each
            # constructor records / touches the optimizer's learning rate)
            ramp = sched_mod.LinearLR(optimizer, start_factor=0.1, total_iters=n_warm)
            main = self.lr_schedulers[name](optimizer, **kwargs)
            scheduler = sched_mod.SequentialLR(optimizer, schedulers=[ramp, main], milestones=[n_warm])
        entry = {"scheduler": scheduler, "monitor": f"val_{self.monitor_metric}"}
        fam = _family(name)
        if fam == "plateau":
            entry.update(reduce_on_plateau=True, strict=False)  # Lightning: step after validation, tolerate a missing metric
        else:
            entry.update(interval="step" if fam == "onecycle" else "epoch", frequency=1)
        return {"optimizer": optimizer, "lr_scheduler": entry}
