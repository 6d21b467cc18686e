"""One rank of the 2-rank world of tests/test_tuner_gpu.py::test_two_ranks_tune_to_the_one_process_rate.  Started by
desco_amd.distributed.launch with the torchrun environment; DESCO_SHARE_GPU=1 puts both ranks on cuda:0 with the gloo
backend, as tests/_multirank_worker.py."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from desco_amd import distributed as D  # noqa: E402


def main():
    out_path = sys.argv[1]
    dev = D.local_device()
    D.init_from_env(dev)
    rank, world = D.rank(), D.world_size()
    assert world == 2
    import tuner_common as T
    from desco_amd import ops
    from desco_amd.trainer import Trainer
    setup = T.Setup(dev)
    model = setup.fresh("neigh")
    if rank == 1:          # a replica that starts elsewhere: tune() must not depend on it, fit() re-synchronises it
        with torch.no_grad():
            for p in model.parameters():
                p.add_(0.25)
    ops.manual_seed(T.SEED)
    tr = Trainer(max_epochs=1, devices=[0, 1], strategy="ddp", default_root_dir=out_path + ".ckpt", auto_lr_find=True)
    out = tr.tune(model, setup.neigh_dm, lr_find_kwargs=dict(T.SWEEP, skip_begin=T.SKIP_BEGIN))
    res = {"lr": model.lr, "args_lr": model.args.lr, "has_record": out["lr_find"] is not None,
           "csv": os.path.exists(out_path + ".ckpt/lr_find.csv")}
    if rank == 0:
        res["raw_loss"] = out["lr_find"].raw_loss
    tr.fit(model, setup.neigh_dm)
    res["history"] = tr.history
    res["params"] = {k: v.cpu() for k, v in T.state(model).items()}
    torch.save(res, f"{out_path}.rank{rank}")
    D.barrier()
    import torch.distributed as dist
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
