"""Rank body of tests/test_gpu_optim.py::test_two_ranks_hold_identical_parameters_and_shadows (started by
robosat_amd.launch.spawn_ranks, in the pattern of tests/dp_worker.py).  ``python optim_dp_worker.py <outdir>``: two replicas on ONE
MI355X (gloo reduces the device tensors through the host) take three native optimiser steps with ``clip_norm`` and ``ema`` on different
shards; every rank writes ``<outdir>/rank<r>.json``."""

import json
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    outdir = sys.argv[1]
    world, rank = int(os.environ["WORLD_SIZE"]), int(os.environ["RANK"])
    from robosat_amd import losses, parallel
    from robosat_amd.optim import AdamW
    from robosat_amd.unet import UNet

    parallel.init_process_group(world, rank, backend="gloo")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(100 + rank)  # every rank draws its own network; the broadcast makes them one
    net = UNet(2, pretrained=False).to(dev).train()
    parallel.broadcast_module(net)
    net.grad_reducer = parallel.GradReducer()  # fp32 on the wire: bit-identical averaged gradients on both ranks
    crit = losses.LovaszLoss2d().to(dev)
    g = torch.Generator().manual_seed(7 + rank)  # different shards
    x = torch.randn(2, 3, 64, 64, generator=g).to(dev)
    t = torch.randint(0, 2, (2, 64, 64), generator=g).to(dev)
    start = [p.detach().clone() for p in net.parameters()]
    # (the shadows are made from the broadcast parameters; clip_norm far below the norm of a fresh network's gradients)
    opt = AdamW(net.parameters(), lr=1e-3, weight_decay=0.01, clip_norm=0.01, ema=0.5,
                schedule={"kind": "poly", "total_steps": 3, "warmup_steps": 1})
    first = None
    for _ in range(3):
        opt.zero_grad()
        loss = crit(net(x), t)
        loss.backward()
        opt.step()
        first = float(loss.detach()) if first is None else first
    torch.cuda.synchronize()

    def same_everywhere(tensors):
        ok = True
        for v in tensors:
            ref = v.detach().clone()
            dist.broadcast(ref, src=0)
            ok = ok and bool(torch.equal(v.detach(), ref))
        return ok

    res = {"params_equal": same_everywhere(list(net.parameters())), "shadows_equal": same_everywhere(opt.shadows),
           "steps": opt.steps_taken(), "coef": float(opt._ctl.view(torch.float32)[4]), "loss_first": first,
           "moved": max(float((p.detach() - s).abs().max()) for p, s in zip(net.parameters(), start)),
           "shadow_differs_from_params": any(not torch.equal(p.detach(), s) for p, s in zip(net.parameters(), opt.shadows))}
    with open(os.path.join(outdir, "rank{}.json".format(rank)), "w") as fp:
        json.dump(res, fp)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
