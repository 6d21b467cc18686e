#!/usr/bin/env python3
"""The ablation WITHOUT canonical partition on the MI355X-native path, with the reference driver's CLI and flow
(ablation_wo_canonical.py of the reference: the third row of the paper's ablation table).  One SHMP model reads WHOLE
target graphs -- no neighborhoods, no canonical node, no gossip stage -- and regresses the graph-level counts:

    ground truth (canonical counts summed per graph) -> WoCanonicalDataset (GraphBatch per graph range, typed CSR
    built on the GPU) -> NeighborhoodCountingModel.to_hetero_wo_canonical (train / load, test, predict)
    -> config_<dataset>.txt + norm-MSE / MAE grouped by query size

``use_hetero``, ``use_tconv``, ``conv_type="SAGE"``, ``use_canonical=False`` are forced and the gossip stage is off,
whatever the command line says (reference :332-338).  Flags: desco_amd/config.py.
"""
from __future__ import annotations

import argparse
import datetime
import os

import numpy as np
import torch
import torch.nn.functional as F

from desco_amd.analysis import mae, norm_mse
from desco_amd.config import parse_gossip, parse_neighborhood, parse_optimizer, split_namespaces
from desco_amd.data import gen_query_ids, graph_atlas_plus, load_data
from desco_amd.lightning_data import LightningDataLoader
from desco_amd.lightning_model import NeighborhoodCountingModel
from desco_amd.trainer import ModelCheckpoint, Trainer
from desco_amd.transforms import ToTconvHetero
from desco_amd.workload import Workload


def build_workload(name, query_ids, nx_queries, transform, num_cpu, root="data", node_feat_len=-1):
    """Target graphs, canonical ground truth (loaded or computed), its per-graph sums, the whole-graph dataset"""
    w = Workload(load_data(name, root_folder=root), os.path.join(root, name), hetero_graph=True,
                 node_feat_len=node_feat_len)
    if w.exist_groundtruth(query_ids=query_ids, queries=nx_queries):
        w.canonical_count_truth = w.load_groundtruth(query_ids=query_ids, queries=nx_queries)
    else:
        w.canonical_count_truth = w.compute_groundtruth(query_ids=query_ids, queries=nx_queries, num_workers=num_cpu,
                                                        save_to_file=True)
    w.canonical_to_graphlet_truth(w.canonical_count_truth)
    w.generate_wo_canonical_dataset(transform=transform)
    return w


def main(args_neighborhood, args_gossip, args_opt, train_neighborhood=True, neighborhood_checkpoint=None,
         nx_queries=None, atlas_query_ids=None, output_dir="results/raw", data_root="data"):
    if nx_queries is None and atlas_query_ids is None:
        raise ValueError("nx_queries and atlas_query_ids cannot be both None")
    query_ids = atlas_query_ids
    use_feat = bool(getattr(args_neighborhood, "use_node_feature", False))
    if nx_queries is None:
        nx_queries = [graph_atlas_plus(i) for i in atlas_query_ids]
        if use_feat:
            from desco_amd.data import add_node_feat_to_networkx
            eye = [t for t in np.eye(args_neighborhood.input_dim).tolist()]
            nx_queries = [g for q in nx_queries for g in add_node_feat_to_networkx(q, eye, "feat")]
            query_ids = None
    else:
        query_ids = None
    node_feat_len = args_neighborhood.input_dim if use_feat else -1
    transform = ToTconvHetero() if args_neighborhood.use_tconv else None
    assert args_neighborhood.use_hetero if args_neighborhood.use_tconv else True
    ncpu = args_opt.num_cpu
    devices = args_opt.gpu if isinstance(args_opt.gpu, list) else [args_opt.gpu]
    if len(devices) > 1:
        raise NotImplementedError("ablation_wo_canonical.py runs on one GPU (--gpu N)")

    train_w = valid_w = None
    if train_neighborhood:
        train_w = build_workload(args_opt.train_dataset, query_ids, nx_queries, transform, ncpu, data_root,
                                 node_feat_len)
        valid_w = build_workload(args_opt.valid_dataset, query_ids, nx_queries, transform, ncpu, data_root,
                                 node_feat_len)
    test_w = build_workload(args_opt.test_dataset, query_ids, nx_queries, transform, ncpu, data_root, node_feat_len)

    loader = LightningDataLoader(
        train_dataset=train_w.wo_canonical_dataset if train_w else None,
        val_dataset=valid_w.wo_canonical_dataset if valid_w else None,
        test_dataset=test_w.wo_canonical_dataset, batch_size=args_neighborhood.batch_size, num_workers=ncpu,
        shuffle=False)
    ckpt = ModelCheckpoint(monitor="neighborhood_counting_val_loss", mode="min", save_top_k=1, save_last=True)
    trainer = Trainer(max_epochs=args_neighborhood.epoch_num, accelerator="gpu", devices=devices,
                      default_root_dir=args_neighborhood.model_path, callbacks=[ckpt], grad_reduce="mean",
                      verbose=True, precision=getattr(args_opt, "precision", "fp32"),
                      auto_lr_find=getattr(args_neighborhood, "tune_lr", False),
                      auto_scale_batch_size=getattr(args_neighborhood, "tune_bs", False))
    if train_neighborhood and neighborhood_checkpoint is None:
        model = NeighborhoodCountingModel(input_dim=args_neighborhood.input_dim,
                                          hidden_dim=args_neighborhood.hidden_dim, args=args_neighborhood)
        model = model.to_hetero_wo_canonical(tconv_target=args_neighborhood.use_tconv,
                                             tconv_query=args_neighborhood.use_tconv)
    else:
        assert neighborhood_checkpoint is not None
        print("loading neighborhood model from checkpoint: ", neighborhood_checkpoint)
        model = NeighborhoodCountingModel.load_from_checkpoint(neighborhood_checkpoint)   # to hetero on loading
    model.to(trainer.device)
    model.set_queries(query_ids=query_ids, queries=nx_queries, transform=transform)
    if train_neighborhood:
        if trainer.auto_lr_find or trainer.auto_scale_batch_size:
            trainer.tune(model=model, datamodule=loader)
        trainer.fit(model=model, datamodule=loader)
        for h in trainer.history:
            if "train_loss" in h:
                print(f"epoch {h['epoch']}: neighborhood_counting_train_loss = {h['train_loss']:.6g}")
        print("best neighborhood model path: ", ckpt.best_model_path)
        model = NeighborhoodCountingModel.load_from_checkpoint(ckpt.best_model_path)
        model.to(trainer.device)
        model.set_queries(query_ids=query_ids, queries=nx_queries, transform=transform)
    print("neighborhood test:", trainer.test(model=model, datamodule=loader))

    # ---------------- outputs ----------------
    os.makedirs(output_dir, exist_ok=True)
    ds = args_opt.test_dataset
    with open(os.path.join(output_dir, f"config_{ds}.txt"), "w") as f:
        f.write(f"args_opt: \n{args_opt}\nargs_neighborhood:\n{args_neighborhood}\nargs_gossip:\n{args_gossip}"
                f"\ntime:\n{datetime.datetime.now()}")
    count_pred = torch.cat(trainer.predict(model, loader.test_dataloader()), dim=0)
    truth = test_w.graphlet_count_truth.cpu().numpy()
    sizes = sorted({len(q) for q in nx_queries})
    groupby = [[i for i, q in enumerate(nx_queries) if len(q) == s] for s in sizes]
    # the dataset's y is log2(count + 1) and the model's own output space adds one more log2(. + 1) on top of it
    # (Workload.generate_wo_canonical_dataset): predict_step has undone the model's, this undoes the dataset's
    count_pred = (2 ** F.relu(count_pred) - 1).cpu().numpy()
    report = {"norm_mse": norm_mse(pred=count_pred, truth=truth, groupby=groupby),
              "mae": mae(pred=count_pred, truth=truth, groupby=groupby)}
    print("norm_mse:", report["norm_mse"])
    print("mae:", report["mae"])
    print("done")
    return report


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description="DeSCo ablation without canonical partition (MI355X-native path)")
    parse_optimizer(parser)
    parse_neighborhood(parser)
    parse_gossip(parser)
    parser.add_argument("--data_root", type=str, default="data")
    parser.add_argument("--precision", type=str, default="fp32", choices=["fp32", "bf16"],
                        help="matrix-product precision of the training steps")
    parser.add_argument("--seed", type=int, default=None,
                        help="seed of the model initialisation (the reference seeds nothing: runs differ)")
    args = parser.parse_args()
    print(args)
    if args.seed is not None:
        import random
        random.seed(args.seed)
        np.random.seed(args.seed)
        torch.manual_seed(args.seed)
    args_neighborhood, args_gossip, args_opt = split_namespaces(args)
    args_opt.precision = args.precision
    # the ablation's model (reference :332-338)
    args_neighborhood.use_hetero = True
    args_neighborhood.use_tconv = True
    args_neighborhood.conv_type = "SAGE"
    args_neighborhood.use_canonical = False
    args_opt.test_gossip = False
    args_opt.train_gossip = False
    output_dir = args_opt.output_dir or os.path.join(
        "results/kdd23/raw", datetime.datetime.now().strftime("%Y%m%d_%H:%M:%S"))
    main(args_neighborhood, args_gossip, args_opt, train_neighborhood=args_opt.train_neigh,
         neighborhood_checkpoint=args_opt.neigh_checkpoint, atlas_query_ids=gen_query_ids(query_size=[3, 4, 5]),
         output_dir=output_dir, data_root=args.data_root)
