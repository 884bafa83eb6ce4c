"""Rank process of tests/test_ema_gpu.py::test_ema_under_data_parallelism (NOT a test module; modelled on _optim_ddp_child.py).

Every rank builds the same C1 model on cuda:0 (the ranks share the one GPU; the collectives run over gloo) and takes STEPS
optimisation steps of FusedSGD on its DistributedSampler share of a fixed batch, dropout off, with `train.ema_decay: 0.9` --
once under each gradient exchange named on the command line, in one process group.  Without a process group (WORLD_SIZE unset)
the one process takes the whole batch.  Rank r writes, per exchange, the parameters and the averaged buffer to <out>/rank{r}.pt."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

STEPS = 3


def run(exchange):
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
        "train": dict(batch_size=8, ep=1, precision="32", ddp_exchange=exchange, ema_decay=0.9),
        "loss": {"name": "mae"}, "opt": {"type": "SGD", "lr": 1e-2, "weight_decay": 0.01}, "data": {"param": "log_g"},
        "noise": {"noise_level": 0},
    }
    module = ViTLModule(config=config)
    module.model.load_state_dict(refvit.make_state_dict(rc, 100 + int(os.environ.get("RANK", "0"))))
    trainer = Trainer(config["train"], device=torch.device("cuda", 0), verbose=False)
    trainer._setup(module)
    module.eval()  # dropout off (masks are per-sample functions of (seed, row): a sharded batch would see other masks)
    flux, error, labels = refvit.make_inputs(rc, 8, 7)
    idx = ddp_mod.shard_indices(8, trainer.rank, trainer.world, epoch=0, shuffle=False)
    batch = tuple(t[idx].cuda() for t in (flux, error, labels))
    eng = module.model.engine
    for i in range(STEPS):
        trainer.training_step(module, batch, i)
    torch.cuda.synchronize()
    avg = trainer.averager
    return {"params": eng.flat.detach().cpu().clone(), "ema": avg.flat.detach().cpu().clone(), "n_averaged": avg.n_averaged,
            "n_trainable": eng.layout.n_trainable, "world": trainer.world,
            "mode": trainer.reducer.mode if trainer.reducer else None}


def main(out_dir, *exchanges):
    out = {ex: run(ex) for ex in exchanges}
    torch.save(out, os.path.join(out_dir, f"rank{int(os.environ.get('RANK', '0'))}.pt"))
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], *sys.argv[2:])
