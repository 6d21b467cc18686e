"""Inputs shared by tests/test_tuner_gpu.py and tests/_tuner_worker.py (its 2-rank side): the same seeded models, graphs,
ground truth and batch streams in every process."""
import functools

import torch

import helpers
from helpers import golden_graphs, make_models, standard_queries

# the sweep of every test: 24 steps from 1e-6 to 1e-1, suggestions read with skip_begin=3
SWEEP = dict(min_lr=1e-6, max_lr=1e-1, num_training=24)
SKIP_BEGIN = 3
SEED = 7                   # ops.manual_seed before every run that is compared with another
NEIGH_DROPOUT, GOSSIP_DROPOUT = 0.1, 0.01
NEIGH_BATCH = 64           # neighborhoods per batch (ragged last batch)
GOSSIP_BATCH = 5           # graphs per batch (12 graphs: 5 + 5 + 2)


class DM:
    """The slice of a datamodule Trainer and lr_find read: re-iterable batch streams, built once on the device."""

    def __init__(self, batches):
        self.b = list(batches)

    def train_dataloader(self):
        return self.b

    def val_dataloader(self):
        return self.b


def _models():
    """helpers.make_models(seed=0) with --neigh_dropout 0.1 / --gossip_dropout 0.01 in the models' args (dropout draws
    nothing at construction: the weights are make_models' own)."""
    na, ga = helpers.neigh_args, helpers.gossip_args
    helpers.neigh_args = functools.partial(na, dropout=NEIGH_DROPOUT)
    helpers.gossip_args = functools.partial(ga, dropout=GOSSIP_DROPOUT)
    try:
        return make_models(seed=0)
    finally:
        helpers.neigh_args, helpers.gossip_args = na, ga


class Setup:
    """12 golden graphs of at most 41 nodes, the 29 standard queries, exact ground truth; the neighborhood stream (y = the
    truth of each neighborhood's node) and the gossip stream (x = the truth off by a seeded factor, y = the truth)."""

    def __init__(self, device):
        from desco_amd.graphs import GraphSet
        from desco_amd.groundtruth import canonical_counts
        from desco_amd.workload import Workload
        self.device = device
        self.qids, queries = standard_queries()
        gs = GraphSet.from_edge_lists(golden_graphs(max_n=41)[:12])
        truth = canonical_counts(gs, queries)
        w = Workload(gs, root=None)
        w.canonical_count_truth = truth
        w.generate_pipeline_datasets(depth_neigh=4)
        self.neigh_dm = DM(w.neighborhood_dataset.batches(NEIGH_BATCH, device))
        g = torch.Generator().manual_seed(11)
        gd = w.gossip_dataset
        gd.x = torch.floor(truth.float() * (0.5 + torch.rand(truth.shape, generator=g)))
        self.gossip_dm = DM(gd.batches(GOSSIP_BATCH, device))
        self.qemb = None

    def dm(self, kind):
        return self.neigh_dm if kind == "neigh" else self.gossip_dm

    def fresh(self, kind):
        """a newly built, identically seeded model of the stage, ready to train"""
        nm, gm = _models()
        nm = nm.to(self.device)
        nm.set_queries(self.qids)
        if kind == "neigh":
            return nm
        if self.qemb is None:
            self.qemb = nm.get_query_emb().detach().clone()
        gm = gm.to(self.device)
        gm.set_query_emb(self.qemb)
        return gm


def state(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}
