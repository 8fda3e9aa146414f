"""One rank of tests/test_failed_step_gpu.py::test_two_ranks_take_the_same_skip_decision: three training steps on this rank's half of a
golden batch with ``ddp.allreduce_gradients(model)`` + ``FusedAdam.step()`` (gloo: all ranks share cuda:0; RCCL: one GPU per rank).  Step 2
is flagged on rank 1 alone.  Every rank runs the same collectives and reaches the final barrier whatever happens in between: a
SpairHipError is caught and recorded, never left to end the process in front of a collective.  Each rank saves what it saw."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

BOX_MEAN_BIAS = "box_network.output_layers.0.bias"


def main():
    prefix, dtype, variant = sys.argv[1], sys.argv[2], sys.argv[3]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    import golden_inputs as gi
    from helpers import load_case
    from spair_pytorch_amd import config as cfg, ddp
    from spair_pytorch_amd._lib import SpairHipError
    from spair_pytorch_amd.models import SPAIR
    from spair_pytorch_amd.optim import FusedAdam
    backend = os.environ.get("SPAIR_DIST_BACKEND", "gloo")
    dev_index = rank if backend == "nccl" else 0
    torch.cuda.set_device(dev_index)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev_index))
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)
    z, case = load_case("c1_b8_step1001")
    cfg.set_grid(case["I"], case["strides"])
    m = SPAIR([1, case["I"], case["I"]], None, torch.device("cuda"), compute_dtype=dtype).to("cuda")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in gi.make_weights(case["wseed"], case["wscale"]).items()})
    overlap = os.environ.get("SPAIR_DDP_OVERLAP", "1") != "0"
    ddp.attach(m, world, overlap=overlap)
    ddp.broadcast_parameters(m.flat_parameters())
    B = z["x"].shape[0]
    lo, hi = rank * B // world, (rank + 1) * B // world
    x = torch.from_numpy(z["x"][lo:hi]).cuda()
    noise = {k: torch.from_numpy(z[k][lo:hi]).cuda() for k in ("eps_box", "eps_attr", "eps_depth", "u_pres")}
    opt = FusedAdam(m, lr=1e-3)
    dec_lo, dec_hi = ddp.GradBuckets(m).ranges[0]
    bias = dict(m.named_parameters())[BOX_MEAN_BIAS]
    out = dict(p0=m.flat_parameters().cpu().numpy())
    skipped = []

    def step(gs, flag):
        opt.zero_grad()
        keep = bias.detach().clone()
        if flag and variant == "natural":
            with torch.no_grad():
                bias[0] = float("nan")             # the cy KL of this forward is NaN, alone (the sampled latent is clamped before use)
        loss = m(x, gs, noise=noise)[0]
        loss.backward()
        if flag:
            g = m.flat_gradients()
            assert torch.isfinite(g[dec_lo:dec_hi]).all() and float(g[dec_lo:dec_hi].abs().max()) > 0       # what the other ranks would apply
            if variant == "natural":
                assert not np.isfinite(loss.item()) and not torch.isfinite(g).all()
                with torch.no_grad():
                    bias.copy_(keep)               # the poison was this forward's: the replicas' parameters are one set again
            else:
                assert torch.isfinite(g).all()
                m._status_dev[1] = 1               # the band-split time-out bit, simulated (never provoked)
            torch.cuda.synchronize()               # a hand-made flag is not ordered in front of the communication stream as the loss kernel's is
        ddp.allreduce_gradients(m)
        opt.step()
        torch.cuda.synchronize()
        skipped.append(opt.skipped()[0])
        n = len(skipped)
        out.update({"p%d" % n: m.flat_parameters().cpu().numpy(), "m%d" % n: opt.exp_avg.cpu().numpy(),
                    "v%d" % n: opt.exp_avg_sq.cpu().numpy()})

    step(1001, False)
    assert m.step_status() == 0
    step(1002, rank == 1)
    message = ""
    try:
        m.check_step_status()
        raised_check = False
    except SpairHipError as e:
        raised_check, message = True, str(e)
    try:
        m(x, 1003, noise=noise)
        raised_forward = False
    except SpairHipError:
        raised_forward = True
    m.clear_step_status()
    step(1003, False)
    np.savez("%s%d.npz" % (prefix, rank), skipped=np.array(skipped), raised_check=raised_check, raised_forward=raised_forward,
             message=message, status3=m.step_status(), **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
