"""Rank process of tests/test_registers_gpu.py::test_two_ranks_stay_bit_identical (NOT a test module; modelled on
_sam_ddp_child.py).

Every rank builds the same C1 model with R register tokens on cuda:0 (the ranks share the one GPU; the collectives run over
gloo) and takes STEPS optimisation steps of the fused AdamW on its DistributedSampler share of a fixed batch, dropout off.  Rank r
writes the parameters and the exchanged gradient of step 1 to <out>/rank{r}.pt.  Without a process group (WORLD_SIZE unset) the
one process instead computes, at the start weights, each shard's own gradient (what each rank had before the exchange)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

STEPS = 2
R = 4
REG = "vit.embeddings.register_tokens"


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
                      num_attention_heads=rc.num_attention_heads, stride_size=rc.stride_size, proj_fn="SW",
                      num_register_tokens=R),
        "train": dict(batch_size=8, ep=1, precision="32", ddp_exchange="allreduce"),
        "loss": {"name": "mae"}, "opt": {"type": "AdamW", "lr": 1e-3}, "data": {"param": "log_g"},
        "noise": {"noise_level": 0},
    }
    module = ViTLModule(config=config)
    sd = refvit.make_state_dict(rc, 100)
    sd[REG] = torch.randn(1, R, rc.hidden_size, generator=torch.Generator().manual_seed(101))
    module.model.load_state_dict(sd)
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
        out["shard_grads"] = []
        for rank in range(2):
            idx = ddp_mod.shard_indices(8, rank, 2, epoch=0, shuffle=False)
            for p in model.parameters():
                p.grad = None
            model(flux[idx].cuda(), labels=labels[idx].cuda()).loss.backward()
            out["shard_grads"].append(eng.grads[:n].detach().cpu().clone())
    else:
        idx = ddp_mod.shard_indices(8, trainer.rank, trainer.world, epoch=0, shuffle=False)
        batch = tuple(t[idx].cuda() for t in (flux, error, labels))
        for i in range(STEPS):
            trainer.training_step(module, batch, i)
            torch.cuda.synchronize()
            if i == 0:
                out["grad_step1"] = eng.grads[:n].detach().cpu().clone()
        out["params"] = eng.flat.detach().cpu().clone()
    torch.save(out, os.path.join(out_dir, f"rank{int(os.environ.get('RANK', '0'))}.pt"))
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
