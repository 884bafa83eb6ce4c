"""One optimisation step of the path as a hipGraph (MI355X-first: HIP streams and graphs instead of a tracing compiler).

A ViT-B step is ~340 kernel launches from Python through ctypes; eagerly the host keeps up, but ~0.7-1 ms of the 42 ms
step were gaps between launches.  Captured once, the step is replayed with one `hipGraphLaunch`.  What changes from step
to step cannot live in kernel arguments (they are frozen at capture), so it lives in device memory the kernels read at
entry: a 32-byte record (`vit_step_state_bind`, include/vit_amd.h) with the dropout keys of the step and Adam's step count /
bias corrections, advanced by the first node of the graph (`vit_step_advance`); and the optimizer's group table with the
learning rates, weight decays and SGD's momenta, which the optimizer rewrites ahead of a replay whenever a scheduler changed
one (`FusedOptimizer._sync_group_table`).  The host writes nothing into the record but the step counter.  With weight
averaging (`train.ema_decay`, vit_amd/ema.py) the update of the average is the graph's last node; its lerp weight -- 0 on a step the
schedule skips, 1 for the first update, 1 - decay otherwise -- lives in a one-float device cell that is rewritten the same way.
Stochastic depth (`model.drop_path_rate`) needs no mechanism of its own: the frozen launches carry each layer's rate p_i, and
the per-sample gate is drawn from the record's keys like every dropout mask, so each replay draws a fresh one.
Patch dropout (`model.patch_drop_rate`) needs nothing new either: the kept count K is frozen in the launches' shapes, and the
subset each sample keeps is drawn by vit_patch_select from the record's keys, so each replay selects afresh.
Masked spectrum modelling (`model.task_type: mim`) rides on the same selection: each replay draws a fresh block mask, and the
loss's denominator -- the number of masked windows, which varies with the mask -- is counted on the device, so nothing on the
host changes from replay to replay.
Global average pooling (`model.global_pool: avg`) adds two nodes, vit_token_pool_fwd / _bwd, whose arguments are shapes alone.
Sharpness-aware minimisation (`train.sam_rho`, vit_amd/sam.py) doubles the body between vit_step_advance and the clip: forward,
backward, the norm of that gradient (vit_sam_sqnorm into a device cell), vit_sam_ascend over [0, n_trainable) -- the range the
optimizer launch covers -- which reads the norm from the cell and keeps the weights in the backup buffer, LayerScale's fold again,
the second forward and backward, vit_sam_descend.  vit_step_advance runs once, so both passes read the same keys from the bound
record: a replay draws the same masks twice and fresh ones on the next replay.  The returned loss is the first pass's.

Scope: one process, one GPU (the RCCL exchange of N > 1 is not captured), a fused optimizer (vit_amd/optimizer.py:
FusedAdamW, FusedLamb, FusedSGD), no trainable input preprocessor, a fixed batch shape.  The reference's step semantics are unchanged
(zero_grad -> forward, dropout on -> backward -> clip the global norm -> optimizer step: src/basemodule.py:230-251); only the
seed schedule of the dropout masks differs from the eager path
(masks are implementation-defined in the reference too).  The eager path stays the default everywhere but bench.py.

torch provides the capture plumbing (`torch.cuda.CUDAGraph` = hipStreamBeginCapture / hipGraphInstantiate / hipGraphLaunch
plus a private allocator pool so tensors created during capture keep their addresses).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _cabi
from . import functional as vf
from .optimizer import FusedOptimizer

__all__ = ["GraphedTrainStep"]


class GraphedTrainStep:
    """`step(batch) -> loss` replaying a captured forward + backward + clip + optimizer update over `module.model` (a MyViT).

    `batch` = (flux, error, labels); tensors whose storage differs from the captured ones are copied into the static input
    buffers first (a device-to-device copy of the batch).  With Mixup / CutMix configured (`module.mixer`) that copy is the
    mix itself: `mixer.apply(flux, labels, out_x=self.x, out_y=self.labels)` ahead of the replay, the same bytes moved.

    Stochastic depth (`model.drop_path_rate`) rides along unchanged: the frozen launches carry each layer's rate, the bound
    record's keys vary the per-sample draw from replay to replay, as they vary the dropout masks."""

    def __init__(self, module, optimizer: FusedOptimizer, batch, warmup: int = 2, averager=None):
        model = module.model
        eng = model.engine
        if not isinstance(optimizer, FusedOptimizer):
            raise TypeError("GraphedTrainStep needs a fused optimizer (FusedAdamW, FusedLamb, FusedSGD)")
        if optimizer._extras or model.preprocessor is not None:
            raise ValueError("GraphedTrainStep: a trainable input preprocessor is outside the captured step")
        if getattr(module, "noise_level", 0):
            raise ValueError("GraphedTrainStep: on-the-fly noise draws a host seed per step; not captured")
        flux, _, labels = batch
        self.module, self.opt, self.eng, self.averager = module, optimizer, eng, averager
        dev = eng.flat.device
        eng._ensure_device_state()
        self.h = eng.handle()  # the engine's own handle: its calls read the bound per-step record
        # per-step device record: [key0, key1 (u32) | reserved | bc1, rsqrt_bc2 (f32) | step (u32) | reserved, reserved]
        self.state = torch.zeros(8, dtype=torch.int32, device=dev)
        self.state[5] = int(optimizer._step)
        self.x = flux.detach().to(dev, torch.float32).contiguous().clone()
        # Mixup / CutMix (module.mixer, vit_amd/mix.py): the mix launches ARE the copy into the static buffers, outside the graph
        # (step()); the label buffer has the shape and dtype of the mixed targets.  The warm-up and the capture draw nothing.
        self.mixer = getattr(module, "mixer", None)
        if self.mixer is not None:
            self.labels = self.mixer.targets_like(labels.detach().to(dev))
        else:
            self.labels = labels.detach().to(dev).contiguous().clone()
        # the copy into the static buffers is skipped only for the very tensor OBJECTS captured, unmodified since (holding the
        # references keeps their storage from being recycled for another batch at the same address)
        self._src = (flux, labels, flux._version, labels._version)
        self.dloss = torch.ones(1, dtype=torch.float32, device=dev)
        self._betas = optimizer._graph_betas()
        optimizer._ensure_state()
        self._captured = optimizer._graph_signature()
        self._tables = optimizer._sync_group_table()  # the capture holds their addresses; `_captured` pins the partition
        module.train()
        # the warm-up steps below are real optimisation steps; parameters, optimizer state and counters are put back afterwards
        # so that the first replay IS the run's next step
        eng._ensure_device_state()
        keep = (eng.flat.clone(), optimizer.clone_state(), int(eng.step_counter))
        if averager is not None:
            averager._ensure()  # the capture holds the addresses of its buffer and of its weight cell
            keep_ema = averager.clone_state()
        self.sam = getattr(model, "sam", None)
        if self.sam is not None:
            self.sam._ensure()  # likewise: the backup buffer and the norm's cell
        # warm-up on a side stream (torch's capture protocol): sizes the arena / workspace, sets the kernels' LDS attributes
        # one stream inside the graph: two-branch graphs (the weight-gradient GEMMs on their second stream) replayed 0.7 ms per
        # step SLOWER than the same two streams launched eagerly on this stack.  The engine's own setting is put back after
        # the capture, so eager steps elsewhere (another batch shape, the bench's instrumented repetition) keep theirs.
        overlap_was = eng.overlap_dw
        eng.overlap_dw = False
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        _cabi.check(self.h.lib.vit_step_state_bind(self.h.h, self.state.data_ptr()), "vit_step_state_bind")
        try:
            with torch.cuda.stream(s):
                for _ in range(max(1, warmup)):
                    self._body()
            torch.cuda.current_stream(dev).wait_stream(s)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.loss = self._body()
            # The graph replays RAW POINTERS into the activation arena and the library workspace.  Hold the tensors: whatever
            # the engine or the handle do later (another batch size, a grown workspace), the captured addresses stay valid and
            # are nobody else's.  (The engine also keeps evaluation forwards in their own arena: engine._ensure_arena.)
            self._held = (eng.act, eng.tmp, self.h._ws, eng._ls)  # _ls: LayerScale's folded operands, slabs and table
            if self.sam is not None:
                self._held += (self.sam.backup, self.sam._sq)
        finally:
            # also on a failed warm-up / capture: the warm-up steps were real optimisation steps and must not leak into the run
            _cabi.check(self.h.lib.vit_step_state_bind(self.h.h, None), "vit_step_state_bind")
            eng.overlap_dw = overlap_was
            torch.cuda.synchronize(dev)
            eng.flat.copy_(keep[0])
            if self.sam is not None:
                self.sam.perturbed = False  # a failure between the two passes: the weights are the kept ones again
            optimizer.restore_state(keep[1])  # in place: the graph holds the state buffers' addresses
            eng.step_counter = keep[2]
            if averager is not None:
                averager.restore_state(keep_ema)  # in place, like the optimizer's
            self.state[5] = int(optimizer._step)
            self._dev_step = int(optimizer._step)  # host mirror of the record's step counter
            if eng.shadow is not None:
                vf.cast_f32_bf16(eng.flat, eng.shadow)
            eng.mark_shadow_fresh()
            torch.cuda.synchronize(dev)

    def _body(self):
        """The captured sequence.  Host-side scalars below (seed, step) are frozen at capture; their per-step versions
        come from the bound device record.  Every call goes through the engine's handle (one workspace, held below)."""
        with vf.use_handle(self.h):
            return self._body_calls()

    def _body_calls(self):
        eng, opt = self.eng, self.opt
        lib, h = self.h.lib, self.h.h
        st = torch.cuda.current_stream(eng.flat.device).cuda_stream
        b1, b2 = self._betas
        _cabi.check(lib.vit_step_advance(h, eng.base_seed, b1, b2, st), "vit_step_advance")
        if eng.layer_scale:
            # LayerScale: the previous replay's optimizer node rewrote W, b and lambda, so the fold of lambda into the
            # out-projection / FC2 operands is a node of the graph in front of the forward, launched unconditionally
            eng.fold_layer_scale()
        loss, _, _, _ = eng.forward(self.x, self.labels, training=True, need_grad=True)
        eng.backward(self.dloss)
        n = eng.layout.n_trainable
        if self.sam is not None:
            # the two-pass step, stated explicitly: perturb by the gradient just formed, evaluate the same function (same record,
            # same keys) at the perturbed weights, restore; `loss` stays the first pass's
            self.sam.ascend(runs=[(0, n)])
            if eng.layer_scale:
                eng.fold_layer_scale()  # from the perturbed weights; the next replay's first node folds from the stepped ones
            eng.forward(self.x, self.labels, training=True, need_grad=True, reuse_step=True)
            eng.backward(self.dloss)
            self.sam.descend()
        sq = None
        if opt._clip is not None:
            sq = vf.grad_sqnorm(eng.grads[:n], out=opt._sq)
            opt.last_grad_norm = sq
        opt._launch(0, n, self._tables, eng.shadow if eng.precision == "bf16" else None, sq, dyn=True)
        if self.averager is not None:
            self.averager.capture_update()
        return loss

    def step(self, batch, step: Optional[int] = None) -> torch.Tensor:
        """`step`: the number (1-based) of the optimizer step this replay is, for the averaging schedule."""
        flux, _, labels = batch
        self.opt._graph_validate(self._captured)  # ValueError before anything is touched: the caller falls back to eager steps
        if self.averager is not None and step is None:
            raise ValueError("GraphedTrainStep.step: the averaging schedule needs the optimizer step's number (step=)")
        if self.mixer is not None:
            # every step draws its own plan, so the captured tensors are never the step's input as they are
            dev = self.x.device
            self.mixer.apply(flux.detach().to(dev), labels.detach().to(dev), out_x=self.x, out_y=self.labels)
            self._src = (None, None, -1, -1)
        else:
            if flux is not self._src[0] or flux._version != self._src[2]:
                self.x.copy_(flux, non_blocking=True)
                self._src = (None, self._src[1], -1, self._src[3])
            if labels is not self._src[1] or labels._version != self._src[3]:
                self.labels.copy_(labels, non_blocking=True)
                self._src = (self._src[0], None, self._src[2], -1)
        self.opt._sync_group_table()  # on the current stream, ahead of the replay: a launch only when a scheduler changed a number
        ema_w = 0.0
        if self.averager is not None:
            ema_w = self.averager.weight_for(step)
            self.averager.set_device_weight(ema_w)  # likewise: a launch only when the weight differs from the last replay's
        if self._dev_step != int(self.opt._step):
            # the record's step counter (Adam's bias corrections, dropout keys) is advanced by THIS graph's replays only: steps
            # taken elsewhere in between -- another captured shape (an epoch's partial last batch), eager steps -- put it back
            # in line with the optimizer's count before the replay reads it
            self.state[5:6].fill_(int(self.opt._step))
            self._dev_step = int(self.opt._step)
        # the bound record is only read by kernels of THIS graph; bind it around the replay so eager calls elsewhere (an
        # evaluation pass between steps) keep their host-seeded masks
        lib, h = self.h.lib, self.h.h
        _cabi.check(lib.vit_step_state_bind(h, self.state.data_ptr()), "vit_step_state_bind")
        self.graph.replay()
        _cabi.check(lib.vit_step_state_bind(h, None), "vit_step_state_bind")
        self.opt._step += 1          # host mirror of the device counter (no sync)
        self._dev_step += 1
        self.eng.step_counter += 1
        self.eng.mark_shadow_fresh()
        if ema_w != 0.0:
            self.averager.n_averaged += 1
        return self.loss

    __call__ = step
