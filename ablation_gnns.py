#!/usr/bin/env python3
"""The ablation WITHOUT heterogeneous message passing on the MI355X-native path, with the reference driver's CLI and flow
(ablation_gnns.py of the reference).  One plain SAGE (or GIN / GCN) model -- one pre_mp and one set of layer weights
for every node and every edge, the anchor marked by node_feature = 1 instead of a node type -- over the neighborhoods of
get_neigh_canonical (the restricted partition), and no gossip stage:

    ground truth (canonical counts) -> Workload(hetero_graph=False) (restricted neighborhoods, built on the GPU, with
    the 0/1 anchor feature) -> NeighborhoodCountingModel(use_hetero=False) (train / load, test, predict)
    -> per-graph sums -> config_<dataset>.txt + norm-MSE / MAE grouped by query size

``use_hetero=False`` and ``use_tconv=False`` are forced and the gossip stage is off, whatever the command line says
(reference :559-566).  ``--neigh_conv_type`` chooses the layer: SAGE (the default, the reference driver's only one), or
the plain baselines GIN and GCN on the fused plain-layer kernel; anything else is refused.  Flags:
desco_amd/config.py.
"""
from __future__ import annotations

import argparse
import datetime
import os

import numpy as np
import pandas as pd
import torch
import torch.nn.functional as F

from desco_amd.analysis import mae, norm_mse
from desco_amd.config import parse_gossip, parse_neighborhood, parse_optimizer, split_namespaces
from desco_amd.data import gen_query_ids, graph_atlas_plus, load_data
from desco_amd.lightning_data import LightningDataLoader
from desco_amd.lightning_model import NeighborhoodCountingModel
from desco_amd.trainer import ModelCheckpoint, Trainer
from desco_amd.workload import Workload


# the layer types of the homogeneous model (the reference driver hard-codes SAGE under a comment about "limited
# implemented scenarios"; its model classes take all three)
ABLATION_CONV_TYPES = ("SAGE", "GIN", "GCN")


def build_workload(name, query_ids, nx_queries, depth, num_cpu, root="data"):
    """Target graphs, canonical ground truth (loaded or computed; it does not depend on the neighborhood definition),
    the restricted neighborhoods with their anchor feature"""
    w = Workload(load_data(name, root_folder=root), os.path.join(root, name), hetero_graph=False)
    if w.exist_groundtruth(query_ids=query_ids, queries=nx_queries):
        w.canonical_count_truth = w.load_groundtruth(query_ids=query_ids, queries=nx_queries)
    else:
        w.canonical_count_truth = w.compute_groundtruth(query_ids=query_ids, queries=nx_queries, num_workers=num_cpu,
                                                        save_to_file=True)
    w.generate_pipeline_datasets(depth_neigh=depth, neighborhood_transform=None)
    return w


def main(args_neighborhood, args_gossip, args_opt, train_neighborhood=True, neighborhood_checkpoint=None,
         nx_queries=None, atlas_query_ids=None, output_dir="results/raw", data_root="data"):
    if nx_queries is None and atlas_query_ids is None:
        raise ValueError("nx_queries and atlas_query_ids cannot be both None")
    conv = getattr(args_neighborhood, "conv_type", "SAGE")
    if conv not in ABLATION_CONV_TYPES:
        raise NotImplementedError(f"--neigh_conv_type {conv}: ablation_gnns.py runs {', '.join(ABLATION_CONV_TYPES)} "
                                  "(GAT and PNACONV are not on the hot path)")
    if conv != "SAGE":
        gpus = args_opt.gpu if isinstance(args_opt.gpu, list) else [args_opt.gpu]
        if getattr(args_neighborhood, "use_node_feature", False) or len(gpus) > 1:
            raise NotImplementedError(f"--neigh_conv_type {conv} runs on one GPU and without --use_node_feature (column 0 "
                                      "of node_feature is the anchor flag of the homogeneous model)")
    if getattr(args_neighborhood, "use_node_feature", False):
        raise NotImplementedError("ablation_gnns.py (hetero_graph=False) together with --use_node_feature is not "
                                  "supported: column 0 of node_feature is the anchor flag of the homogeneous model")
    query_ids = atlas_query_ids if nx_queries is None else None
    if nx_queries is None:
        nx_queries = [graph_atlas_plus(i) for i in atlas_query_ids]
    depth, ncpu = args_neighborhood.depth, args_opt.num_cpu
    devices = args_opt.gpu if isinstance(args_opt.gpu, list) else [args_opt.gpu]
    if len(devices) > 1:
        raise NotImplementedError("ablation_gnns.py runs on one GPU (--gpu N)")

    train_w = valid_w = None
    if train_neighborhood:
        train_w = build_workload(args_opt.train_dataset, query_ids, nx_queries, depth, ncpu, data_root)
        valid_w = build_workload(args_opt.valid_dataset, query_ids, nx_queries, depth, ncpu, data_root)
    test_w = build_workload(args_opt.test_dataset, query_ids, nx_queries, depth, ncpu, data_root)

    loader = LightningDataLoader(
        train_dataset=train_w.neighborhood_dataset if train_w else None,
        val_dataset=valid_w.neighborhood_dataset if valid_w else None,
        test_dataset=test_w.neighborhood_dataset, batch_size=args_neighborhood.batch_size, num_workers=ncpu,
        shuffle=False)
    ckpt = ModelCheckpoint(monitor="neighborhood_counting_val_loss", mode="min", save_top_k=1, save_last=True)
    trainer = Trainer(max_epochs=args_neighborhood.epoch_num, accelerator="gpu", devices=devices,
                      default_root_dir=args_neighborhood.model_path, callbacks=[ckpt], grad_reduce="mean",
                      verbose=True, precision=getattr(args_opt, "precision", "fp32"),
                      auto_lr_find=getattr(args_neighborhood, "tune_lr", False),
                      auto_scale_batch_size=getattr(args_neighborhood, "tune_bs", False))
    if train_neighborhood and neighborhood_checkpoint is None:
        # (no to_hetero: the model stays homogeneous and keeps the reference's single-module state dict)
        model = NeighborhoodCountingModel(input_dim=args_neighborhood.input_dim,
                                          hidden_dim=args_neighborhood.hidden_dim, args=args_neighborhood)
    else:
        assert neighborhood_checkpoint is not None
        print("loading neighborhood model from checkpoint: ", neighborhood_checkpoint)
        model = NeighborhoodCountingModel.load_from_checkpoint(neighborhood_checkpoint)
    model.to(trainer.device)
    model.set_queries(query_ids=query_ids, queries=nx_queries, transform=None, hetero=False)
    if train_neighborhood:
        if trainer.auto_lr_find or trainer.auto_scale_batch_size:
            trainer.tune(model=model, datamodule=loader)
        trainer.fit(model=model, datamodule=loader)
        for h in trainer.history:
            if "train_loss" in h:
                print(f"epoch {h['epoch']}: neighborhood_counting_train_loss = {h['train_loss']:.6g}")
        print("final neighborhood_counting_val_loss: {:.6g}".format(trainer.history[-1]["neighborhood_counting_val_loss"]))
        print("best neighborhood model path: ", ckpt.best_model_path)
        model = NeighborhoodCountingModel.load_from_checkpoint(ckpt.best_model_path)
        model.to(trainer.device)
        model.set_queries(query_ids=query_ids, queries=nx_queries, transform=None, hetero=False)
    print("neighborhood test:", trainer.test(model=model, datamodule=loader))

    # ---------------- outputs ----------------
    os.makedirs(output_dir, exist_ok=True)
    ds = args_opt.test_dataset
    with open(os.path.join(output_dir, f"config_{ds}.txt"), "w") as f:
        f.write(f"args_opt: \n{args_opt}\nargs_neighborhood:\n{args_neighborhood}\nargs_gossip:\n{args_gossip}"
                f"\ntime:\n{datetime.datetime.now()}")
    neigh_count = torch.cat(trainer.predict(model, loader.test_dataloader()), dim=0)
    graphlet = test_w.neighborhood_dataset.aggregate_neighborhood_count(neigh_count)
    truth = test_w.gossip_dataset.aggregate_neighborhood_count(test_w.canonical_count_truth).numpy()
    sizes = sorted({len(q) for q in nx_queries})
    groupby = [[i for i, q in enumerate(nx_queries) if len(q) == s] for s in sizes]
    pred = torch.round(F.relu(graphlet)).cpu().numpy()
    pd.DataFrame(pred).to_csv(os.path.join(output_dir, f"neighborhood_graphlet_{ds}.csv"))
    pd.DataFrame(neigh_count.cpu().numpy()).to_csv(os.path.join(output_dir, f"neighborhood_node_{ds}_results.csv"))
    pd.DataFrame(test_w.neighborhood_dataset.nx_neighs_index).to_csv(
        os.path.join(output_dir, f"neighborhood_node_{ds}_index.csv"))
    report = {"graphlet_norm_mse_neighborhood": norm_mse(pred=pred, truth=truth, groupby=groupby),
              "graphlet_mae_neighborhood": mae(pred=pred, truth=truth, groupby=groupby),
              "neigh_count": neigh_count}
    print("graphlet_norm_mse_neighborhood:", report["graphlet_norm_mse_neighborhood"])
    print("graphlet_mae_neighborhood:", report["graphlet_mae_neighborhood"])
    with open(os.path.join(output_dir, f"config_{ds}.txt"), "a") as f:
        f.write("\ngraphlet_norm_mse_neighborhood: {}\ngraphlet_mae_neighborhood: {}\n".format(
            report["graphlet_norm_mse_neighborhood"], report["graphlet_mae_neighborhood"]))
    print("done")
    return report


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description="DeSCo ablation without heterogeneous message passing "
                                                 "(MI355X-native path)")
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
    # the ablation's model (reference :559-566)
    args_neighborhood.use_hetero = False
    args_neighborhood.use_tconv = False
    # (--neigh_conv_type is honoured: SAGE by default, GIN or GCN for the plain baselines; main() refuses anything else)
    args_opt.test_gossip = False
    args_opt.train_gossip = False
    output_dir = args_opt.output_dir or os.path.join(
        "results/kdd23/raw", datetime.datetime.now().strftime("%Y%m%d_%H:%M:%S"))
    main(args_neighborhood, args_gossip, args_opt, train_neighborhood=args_opt.train_neigh,
         neighborhood_checkpoint=args_opt.neigh_checkpoint, atlas_query_ids=gen_query_ids(query_size=[3, 4, 5]),
         output_dir=output_dir, data_root=args.data_root)
