"""Rank process of tests/test_sam_gpu.py::test_two_ranks_exchange_the_second_gradient_only (NOT a test module; modelled on
_ema_ddp_child.py).

Every rank builds the same C1 model on cuda:0 (the ranks share the one GPU; the collectives run over gloo) and takes STEPS
optimisation steps of FusedSGD with `train.sam_rho` on its DistributedSampler share of a fixed batch, dropout off.  A spy in front
of the engine's gradient-ready callback counts the buckets handed to the exchange per step.  Rank r writes the parameters, the
exchanged gradient of step 1 and the counts to <out>/rank{r}.pt.  Without a process group (WORLD_SIZE unset) the one process
instead computes, at the start weights, each shard's own plain and sharpness-aware gradient (what each rank had before the
exchange)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

STEPS = 2
RHO = 0.005


def main(out_dir):
    from oracle import refvit  # checker-side helper: seeded weights / inputs only
    from vit_amd import ddp as ddp_mod
    from vit_amd.module import ViTLModule
    from vit_amd.trainer import Trainer, seed_everything

    seed_everything(42)
    rc = refvit.named_config("C1")
    config = {
        "model": dict(name="vit", task_type="reg", image_size=rc.image_size, patch_size=rc.patch_size,
                      hidden_size=rc.hidden_size, num_hidden_layers=rc.num_hidden_layers,
                      num_attention_heads=rc.num_attention_heads, stride_size=rc.stride_size, proj_fn="SW"),
        "train": dict(batch_size=8, ep=1, precision="32", ddp_exchange="allreduce", sam_rho=RHO),
        "loss": {"name": "mae"}, "opt": {"type": "SGD", "lr": 1e-2, "weight_decay": 0.01}, "data": {"param": "log_g"},
        "noise": {"noise_level": 0},
    }
    module = ViTLModule(config=config)
    module.model.load_state_dict(refvit.make_state_dict(rc, 100))
    trainer = Trainer(config["train"], device=torch.device("cuda", 0), verbose=False)
    trainer._setup(module)
    module.eval()  # dropout off (masks are per-sample functions of (seed, row): a sharded batch would see other masks)
    flux, error, labels = refvit.make_inputs(rc, 8, 7)
    eng, model = module.model.engine, module.model
    lay = eng.layout
    n = lay.n_trainable
    out = {"world": trainer.world, "n_trainable": n}
    if trainer.world == 1:
        eng._ensure_device_state()
        out["start"] = eng.flat.detach().cpu().clone()
        out["spans"] = {k: (off, off + lay.numel(k)) for k, (off, _) in lay.entries.items() if off < n}
        out["shard_grads"], out["shard_plain"] = [], []
        for rank in range(2):
            idx = ddp_mod.shard_indices(8, rank, 2, epoch=0, shuffle=False)
            x, y = flux[idx].cuda(), labels[idx].cuda()
            for attach, key in ((True, "shard_grads"), (False, "shard_plain")):
                model.set_sam(RHO if attach else None)
                for p in model.parameters():
                    p.grad = None
                model(x, labels=y).loss.backward()
                out[key].append(eng.grads[:n].detach().cpu().clone())
    else:
        idx = ddp_mod.shard_indices(8, trainer.rank, trainer.world, epoch=0, shuffle=False)
        batch = tuple(t[idx].cuda() for t in (flux, error, labels))
        calls, real = [], eng.grad_ready_cb

        def spy(lo, hi):
            calls.append((lo, hi))
            real(lo, hi)

        eng.grad_ready_cb = spy
        counts = []
        for i in range(STEPS):
            before = len(calls)
            trainer.training_step(module, batch, i)
            torch.cuda.synchronize()
            counts.append(len(calls) - before)
            if i == 0:
                out["grad_step1"] = eng.grads[:n].detach().cpu().clone()
        out.update(params=eng.flat.detach().cpu().clone(), bucket_calls=counts, n_buckets=len(lay.buckets()),
                   perturbed=model.sam.perturbed)
    torch.save(out, os.path.join(out_dir, f"rank{int(os.environ.get('RANK', '0'))}.pt"))
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
