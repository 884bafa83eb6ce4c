"""Rank process of tests/test_lamb_gpu.py::test_two_ranks_stay_bit_identical (NOT a test module; modelled on _optim_ddp_child.py).

Every rank builds the same C1 model on cuda:0 (the ranks share the one GPU; the collectives run over gloo) and takes STEPS
optimisation steps of FusedLamb (`opt.type: lamb` with no-decay and layer-decay groups, clipped) on its DistributedSampler share
of a fixed batch, dropout off, under the all-reduce exchange.  Rank r writes the parameters, both moments, the trust ratios
and the clipping norm of every step to <out>/rank{r}.pt."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

STEPS = 3


def main(out_dir):
    from oracle import refvit  # checker-side helper: seeded weights / inputs only
    from vit_amd import ddp as ddp_mod
    from vit_amd.module import ViTLModule
    from vit_amd.optimizer import FusedLamb
    from vit_amd.trainer import Trainer, seed_everything

    seed_everything(42)
    rc = refvit.named_config("C1")
    config = {
        "model": dict(name="vit", task_type="reg", image_size=rc.image_size, patch_size=rc.patch_size,
                      hidden_size=rc.hidden_size, num_hidden_layers=rc.num_hidden_layers,
                      num_attention_heads=rc.num_attention_heads, stride_size=rc.stride_size, proj_fn="SW"),
        "train": dict(batch_size=8, ep=1, precision="32", ddp_exchange="allreduce", grad_clip=0.5),
        "loss": {"name": "mae"},
        "opt": {"type": "lamb", "lr": 2e-3, "weight_decay": 0.05, "no_decay": True, "layer_decay": 0.75, "always_adapt": True},
        "data": {"param": "log_g"}, "noise": {"noise_level": 0},
    }
    module = ViTLModule(config=config)
    module.model.load_state_dict(refvit.make_state_dict(rc, 100 + int(os.environ.get("RANK", "0"))))
    trainer = Trainer(config["train"], device=torch.device("cuda", 0), verbose=False)
    trainer._setup(module)
    opt = trainer.optimizer
    assert type(opt) is FusedLamb, type(opt)
    module.eval()  # dropout off (masks are per-sample functions of (seed, row): a sharded batch would see other masks)
    flux, error, labels = refvit.make_inputs(rc, 8, 7)
    idx = ddp_mod.shard_indices(8, trainer.rank, trainer.world, epoch=0, shuffle=False)
    batch = tuple(t[idx].cuda() for t in (flux, error, labels))
    eng = module.model.engine
    start = eng.flat.detach().cpu().clone()
    norms = []
    for i in range(STEPS):
        trainer.training_step(module, batch, i)
        norms.append(float(opt.last_grad_norm.sqrt()) if opt.last_grad_norm is not None else None)
    torch.cuda.synchronize()
    names, ratios = opt.last_trust_ratios
    out = {"params": eng.flat.detach().cpu().clone(), "start": start, "m": opt._m.detach().cpu().clone(),
           "v": opt._v.detach().cpu().clone(), "trust": ratios.detach().cpu().clone(), "names": list(names), "norms": norms,
           "n_trainable": eng.layout.n_trainable, "world": trainer.world, "steps": opt._step,
           "mode": trainer.reducer.mode if trainer.reducer else None}
    torch.save(out, os.path.join(out_dir, f"rank{int(os.environ.get('RANK', '0'))}.pt"))
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
