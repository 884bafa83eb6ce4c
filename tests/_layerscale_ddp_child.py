"""Rank process of tests/test_layerscale_gpu.py::test_two_ranks_exchange_true_gradients (NOT a test module; modelled on
_ema_ddp_child.py).

Every rank builds the same C1 model with LayerScale on (lambda = 0.5, seeded biases) on cuda:0 -- the ranks share the one GPU,
the collectives run over gloo -- and takes STEPS optimisation steps of FusedSGD on its DistributedSampler share of a fixed
batch, dropout off, under the all-reduce exchange.  In the last step it keeps a copy of every layer bucket as the engine hands
it to the exchange: the rank's LOCAL gradients.  Rank r writes the parameters, the exchanged gradient buffer and, per lambda,
its local and its exchanged gradient to <out>/rank{r}.pt."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

STEPS = 2


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
                      num_attention_heads=rc.num_attention_heads, stride_size=rc.stride_size, proj_fn="SW", layer_scale_init=0.5),
        "train": dict(batch_size=8, ep=1, precision="32", ddp_exchange="allreduce"),
        "loss": {"name": "mae"}, "opt": {"type": "SGD", "lr": 1e-2, "weight_decay": 0.01}, "data": {"param": "log_g"},
        "noise": {"noise_level": 0},
    }
    module = ViTLModule(config=config)
    sd = refvit.make_state_dict(rc, 100 + int(os.environ.get("RANK", "0")))  # rank 0's weights are broadcast
    gen = torch.Generator().manual_seed(3)
    sd = {k: (0.02 * torch.randn(v.shape, generator=gen) if k.endswith(".bias") else v) for k, v in sd.items()}
    module.model.load_state_dict(sd, strict=False)
    trainer = Trainer(config["train"], device=torch.device("cuda", 0), verbose=False)
    trainer._setup(module)
    module.eval()  # dropout off (masks are per-sample functions of (seed, row): a sharded batch would see other masks)
    flux, error, labels = refvit.make_inputs(rc, 8, 7)
    idx = ddp_mod.shard_indices(8, trainer.rank, trainer.world, epoch=0, shuffle=False)
    batch = tuple(t[idx].cuda() for t in (flux, error, labels))
    eng = module.model.engine
    params0 = eng.flat.detach().cpu().clone()
    handed = {}
    exchange = eng.grad_ready_cb

    def spy(lo, hi):  # on the stream the exchange is enqueued from, in front of it
        handed[(lo, hi)] = eng.grads[lo:hi].clone()
        exchange(lo, hi)

    for i in range(STEPS):
        if i == STEPS - 1:
            eng.grad_ready_cb = spy
        trainer.training_step(module, batch, i)
    torch.cuda.synchronize()
    names = [n for n in module.model._param_names if n.endswith(".lambda1")]
    local, exchanged = {}, {}
    for n in names:
        off, _ = eng.layout.entries[n]
        (lo, hi), buf = next((k, v) for k, v in handed.items() if k[0] <= off < k[1])
        local[n] = buf[off - lo:off - lo + eng.layout.numel(n)].cpu().clone()
        exchanged[n] = eng.g(n).detach().cpu().clone()
    torch.save({"params": eng.flat.detach().cpu().clone(), "params0": params0,
                "grads": eng.grads[:eng.layout.n_trainable].detach().cpu().clone(), "lambda_names": names, "local": local,
                "exchanged": exchanged, "world": trainer.world, "global_step": trainer.global_step},
               os.path.join(out_dir, f"rank{int(os.environ.get('RANK', '0'))}.pt"))
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
