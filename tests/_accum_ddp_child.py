"""Rank process of tests/test_accum_gpu.py::test_ddp_* (started by vit_amd.launch.launch_ranks, or alone as the single-process
comparison; NOT a test module).

Every rank builds the same C1 model on cuda:0 (the ranks share the one GPU of the box and exchange over gloo, as in
tests/_ddp_child.py), and runs ONE optimizer step of `Trainer.training_step` over the same 8 seeded samples with dropout off:
  world 1, K = 1: one batch of 8;
  world W, K    : K micro-batches of 8 / (W * K) samples per rank -- micro-batch m covers the samples [m * 8 / K, (m + 1) * 8 / K),
                  rank r takes every W-th of them.  Equal sizes everywhere, so the mean of the K * W means is the mean over 8.
Rank r writes to <out>/rank{r}.pt: the flat gradient as it was handed to the optimizer, the updated parameters, and the number
of collectives the reducer launched (counted twice: by the reducer itself and by a wrapper around torch.distributed)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch


def main(out_dir, precision, exchange, K):
    from oracle import refvit  # checker-side helper: seeded weights / inputs only
    from vit_amd.module import ViTLModule
    from vit_amd.trainer import Trainer, seed_everything

    K = int(K)
    seed_everything(42)
    rc = refvit.named_config("C1")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    per_rank = 8 // (world * K)
    config = {
        "model": dict(name="vit", task_type="reg", image_size=rc.image_size, patch_size=rc.patch_size,
                      hidden_size=rc.hidden_size, num_hidden_layers=rc.num_hidden_layers,
                      num_attention_heads=rc.num_attention_heads, stride_size=rc.stride_size, proj_fn="SW"),
        "train": dict(batch_size=per_rank, ep=1, precision=precision, ddp_exchange=exchange, accumulate_grad_batches=K),
        "loss": {"name": "mae"}, "opt": {"type": "AdamW", "lr": 1e-3}, "data": {"param": "log_g"}, "noise": {"noise_level": 0},
    }
    module = ViTLModule(config=config)
    module.model.load_state_dict(refvit.make_state_dict(rc, 100 + int(os.environ.get("RANK", "0"))))
    trainer = Trainer(config["train"], device=torch.device("cuda", 0), verbose=False)
    trainer._setup(module)
    module.eval()  # dropout off (masks are functions of (seed, row): a split batch would see other masks)
    flux, error, labels = refvit.make_inputs(rc, 8, 7)
    eng = module.model.engine
    seen = {}
    step0 = trainer.optimizer.step

    def spy_step(*a, **k):
        seen["grads"] = eng.grads.detach().cpu().clone()  # after reducer.finish(): what the optimizer consumes
        return step0(*a, **k)

    trainer.optimizer.step = spy_step
    launched = {"n": 0}
    if torch.distributed.is_initialized():
        ar0 = torch.distributed.all_reduce

        def counting_all_reduce(*a, **k):
            launched["n"] += 1
            return ar0(*a, **k)

        torch.distributed.all_reduce = counting_all_reduce
    for m in range(K):
        idx = torch.arange(m * (8 // K) + trainer.rank, (m + 1) * (8 // K), world)
        batch = tuple(t[idx].cuda() for t in (flux, error, labels))
        trainer.training_step(module, batch, m, is_last=False)
        if m < K - 1:
            assert "grads" not in seen and trainer.global_step == 0 and launched["n"] == 0, (m, launched)
    torch.cuda.synchronize()
    lay = eng.layout
    held = all(p.grad is not None and p.grad.data_ptr() == eng.g(n).data_ptr()
               for n, p in zip(module.model._param_names, module.model._param_list) if lay.entries[n][0] < lay.n_trainable)
    torch.save({"grads": seen["grads"], "params": eng.flat.detach().cpu().clone(), "n_trainable": lay.n_trainable,
                "world": trainer.world, "mode": trainer.reducer.mode if trainer.reducer else None,
                "buckets": trainer.reducer.calls_per_step if trainer.reducer else 0,
                "collectives": trainer.reducer.collectives if trainer.reducer else 0, "all_reduce_calls": launched["n"],
                "global_step": trainer.global_step, "opt_step": trainer.optimizer._step, "grads_are_views": held,
                "grad_norm": float(trainer.optimizer.last_grad_norm.sqrt())},
               os.path.join(out_dir, f"rank{trainer.rank}.pt"))
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(*sys.argv[1:5])
