"""The learning-rate range test (desco_amd/tuner.py, Trainer.tune, main.py --neigh_tune_lr / --gossip_tune_lr) on the
GPU: the sweep runs the native training step and leaves no trace -- parameters, the dropout stream, the training that
follows, eager or replayed from hipGraphs, are bit for bit what they are without it; its record is what the
specification says; it is deterministic; Trainer.tune applies and records the suggestion, on one rank and on two;
main.py runs it end to end.  Sweeps of 24 steps from 1e-6 to 1e-1 on 12 golden graphs (tests/tuner_common.py)."""
import csv
import os
import re
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from desco_amd import autograd as AG  # noqa: E402
from desco_amd import distributed as D  # noqa: E402
from desco_amd import ops, tuner  # noqa: E402
from desco_amd.trainer import Trainer  # noqa: E402

import tuner_common as T  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def setup():
    return T.Setup(DEV)


def _fit(setup, kind, root, capture, sweep):
    """(history, state dict, rng words) of Trainer(max_epochs=2).fit on a fresh model of the stage, after a sweep or not"""
    m = setup.fresh(kind)
    ops.manual_seed(T.SEED)
    tr = Trainer(max_epochs=2, default_root_dir=str(root), graph_capture=capture)
    res = None
    if sweep:
        before, rng = T.state(m), ops.rng_state(DEV).clone()
        lr0, training = m.lr, m.training
        res = tuner.lr_find(tr, m, setup.dm(kind), update_attr=False, **T.SWEEP)
        torch.cuda.synchronize()
        after = T.state(m)
        for k in before:
            assert torch.equal(before[k], after[k]), k
        assert torch.equal(rng, ops.rng_state(DEV)) and ops.rng_state(DEV).tolist()[0] == T.SEED
        assert m.lr == lr0 and m.training == training and all(p.grad is None for p in m.parameters())
    tr.fit(m, setup.dm(kind))
    torch.cuda.synchronize()
    return tr.history, T.state(m), ops.rng_state(DEV).tolist(), res


@pytest.fixture(scope="module")
def plain_fits(setup, tmp_path_factory):
    """the fits WITHOUT a sweep, one per (stage, capture), computed on first use and shared"""
    cache = {}

    def get(kind, capture):
        if (kind, capture) not in cache:
            cache[kind, capture] = _fit(setup, kind, tmp_path_factory.mktemp(f"plain_{kind}_{int(capture)}"), capture,
                                        sweep=False)[:3]
        return cache[kind, capture]
    return get


@pytest.fixture(scope="module")
def record(setup):
    """one sweep of the neighborhood model from (fresh weights, seed 7): the record the later tests read"""
    m = setup.fresh("neigh")
    ops.manual_seed(T.SEED)
    return tuner.lr_find(Trainer(max_epochs=1), m, setup.neigh_dm, **T.SWEEP)


# ---- 1 / 5: the sweep leaves no trace -------------------------------------------------------------------------------
@pytest.mark.parametrize("capture", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("kind", ["neigh", "gossip"])
def test_sweep_leaves_no_trace(setup, plain_fits, tmp_path, kind, capture):
    """Neighborhood model at dropout 0.1, gossip model at 0.01.  After lr_find every parameter and the (seed, step) words
    of the dropout stream equal their values before (asserted in _fit), and the 2-epoch fit that follows -- eager, or
    with graph_capture=True, under which the sweep itself still runs eagerly -- gives the history, the weights and the
    dropout counter of the same fit on a fresh identically seeded model that was never swept, bit for bit."""
    hist, sd, rng, res = _fit(setup, kind, tmp_path, capture, sweep=True)
    n = len(res.raw_loss)
    print(f"[tuner] {kind} sweep: {n} steps, raw loss {res.raw_loss[0]:.6g} -> {res.raw_loss[-1]:.6g}, "
          f"stopped early: {res.stopped_early}")
    assert n >= 3 and len(set(res.raw_loss)) == n               # the sweep did train: no two steps saw the same loss
    ref_hist, ref_sd, ref_rng = plain_fits(kind, capture)
    assert len(hist) == 2 and hist == ref_hist
    assert rng == ref_rng and rng[1] > 0                        # dropout keys were drawn, the same number of them
    for k in ref_sd:
        assert torch.equal(sd[k], ref_sd[k]), k
    moved = max(float((sd[k] - v).abs().max()) for k, v in T.state(setup.fresh(kind)).items())
    assert moved > 1e-5                                         # and the fit did train


# ---- 2: the record --------------------------------------------------------------------------------------------------
def test_record_is_what_the_specification_says(setup, record):
    lr, loss, raw = record.results["lr"], record.results["loss"], record.raw_loss
    n = len(raw)
    print(f"[tuner] record: {n} steps, stopped early: {record.stopped_early}, suggestion "
          f"{record.suggestion(skip_begin=T.SKIP_BEGIN)}")
    assert len(lr) == len(loss) == n and 1 <= n <= 24
    assert record.stopped_early == (n < 24)
    assert lr == tuner.sweep_lrs(**T.SWEEP, mode="exponential")[:n]
    # step 0 is one plain training step on the first batch from the same state
    m = setup.fresh("neigh")
    ops.manual_seed(T.SEED)
    AG.set_precision("fp32")
    m.train()
    first = float(m.training_step(setup.neigh_dm.b[0], 0).detach())
    assert raw[0] == first and np.isfinite(first)
    sm, kept = tuner.smooth_and_stop(raw)
    assert kept == n
    np.testing.assert_allclose(loss, sm, rtol=1e-12, atol=0)
    s = record.suggestion(skip_begin=T.SKIP_BEGIN)
    assert s == tuner.suggest(lr, loss, skip_begin=T.SKIP_BEGIN, skip_end=1)
    assert s is not None and T.SWEEP["min_lr"] <= s <= T.SWEEP["max_lr"] and s in lr


# ---- 3: deterministic -----------------------------------------------------------------------------------------------
def test_sweep_is_deterministic(setup, record):
    """the same state and seed give the same raw losses bit for bit: on a fresh model, and again on that same model,
    which the first sweep restored"""
    m = setup.fresh("neigh")
    tr = Trainer(max_epochs=1)
    for _ in range(2):
        ops.manual_seed(T.SEED)
        again = tuner.lr_find(tr, m, setup.neigh_dm, **T.SWEEP)
        assert again.raw_loss == record.raw_loss
        assert again.results == record.results and again.stopped_early == record.stopped_early


# ---- 4: Trainer.tune ------------------------------------------------------------------------------------------------
def test_trainer_tune_applies_and_records_the_suggestion(setup, record, tmp_path, capsys):
    m = setup.fresh("neigh")
    ops.manual_seed(T.SEED)
    tr = Trainer(max_epochs=1, default_root_dir=str(tmp_path / "ck"), auto_lr_find=True)
    out = tr.tune(m, setup.neigh_dm, lr_find_kwargs=dict(T.SWEEP, skip_begin=T.SKIP_BEGIN))
    res = out["lr_find"]
    s = res.suggestion(skip_begin=T.SKIP_BEGIN)
    assert set(out) == {"lr_find"} and res.raw_loss == record.raw_loss
    assert s is not None and s != 1e-4 and m.lr == s and m.args.lr == s and m.hparams_dict["args"].lr == s
    assert str(s) in capsys.readouterr().out
    rows = list(csv.reader(open(tmp_path / "ck" / "lr_find.csv")))
    assert len(rows) == len(res.raw_loss) + 1 and rows[0] == ["step", "lr", "raw_loss", "loss"]
    assert [float(r[2]) for r in rows[1:]] == res.raw_loss
    tr.fit(m, setup.neigh_dm)
    assert tr.history[0]["lr"] == s


def test_trainer_tune_without_its_flags_does_nothing(setup, tmp_path):
    m = setup.fresh("gossip")
    before, rng = T.state(m), ops.rng_state(DEV).clone()
    tr = Trainer(max_epochs=1, default_root_dir=str(tmp_path / "ck"))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert tr.tune(m, setup.gossip_dm) == {}
    tr = Trainer(max_epochs=1, default_root_dir=str(tmp_path / "ck"), auto_scale_batch_size=True)
    with pytest.warns(UserWarning, match="tune_bs|auto_scale_batch_size"):
        assert tr.tune(m, setup.gossip_dm) == {}
    assert m.lr == 1e-3 and m.hparams_dict["args"].lr == 1e-3 and m.hparams_dict["args"].batch_size == 256
    assert torch.equal(rng, ops.rng_state(DEV)) and not (tmp_path / "ck" / "lr_find.csv").exists()
    after = T.state(m)
    assert all(torch.equal(before[k], after[k]) for k in before)


# ---- 6: two ranks ---------------------------------------------------------------------------------------------------
def test_two_ranks_tune_to_the_one_process_rate(record, tmp_path):
    """2 ranks on the one GPU (DESCO_SHARE_GPU=1, gloo, as tests/test_multirank_gpu.py): rank 0 sweeps alone, rank 1 --
    whose replica starts from other weights -- waits for the suggestion; both end with the rate the one-process sweep
    suggests, bit for bit, and the data-parallel fit that follows completes with the replicas in sync."""
    out = str(tmp_path / "tune")
    rc = D.launch([os.path.join(ROOT, "tests", "_tuner_worker.py"), out], 2, env=dict(os.environ, DESCO_SHARE_GPU="1"),
                  timeout=600)
    assert rc == 0, f"2-rank worker failed with exit code {rc}"
    r0, r1 = (torch.load(f"{out}.rank{r}", weights_only=False) for r in (0, 1))
    s = record.suggestion(skip_begin=T.SKIP_BEGIN)
    print(f"[tuner] 2 ranks: lr {r0['lr']} / {r1['lr']}, one process {s}")
    assert r0["raw_loss"] == record.raw_loss
    assert s is not None and r0["lr"] == s and r1["lr"] == s and r0["args_lr"] == s and r1["args_lr"] == s
    assert r0["has_record"] and not r1["has_record"] and r0["csv"]
    assert len(r0["history"]) == 1 and r0["history"] == r1["history"] and r0["history"][0]["lr"] == s
    assert np.isfinite(r0["history"][0]["neighborhood_counting_val_loss"])
    for k in r0["params"]:
        assert torch.equal(r0["params"][k], r1["params"][k]), k


# ---- 7: main.py -----------------------------------------------------------------------------------------------------
def test_main_runs_the_range_test_for_both_stages(tmp_path):
    """main.py --neigh_tune_lr --gossip_tune_lr on toy TU data (as tests/test_main_gpu.py): the default sweep (100 steps,
    1e-8 to 1) runs before each fit, both records are written under the model paths, and config_<dataset>.txt and the
    checkpoints' hyper-parameters carry the rates that were used instead of the defaults 1e-4 / 1e-3."""
    import argparse
    import main as driver
    from desco_amd import config
    from desco_amd.ckpt import load_checkpoint
    from desco_amd.data import STANDARD_QUERY_IDS
    from helpers import golden_graphs
    from test_main_gpu import _write_tu
    root = str(tmp_path / "data")
    _write_tu(root, "TOY", golden_graphs(max_n=30))
    p = argparse.ArgumentParser()
    config.parse_optimizer(p)
    config.parse_neighborhood(p)
    config.parse_gossip(p)
    args = p.parse_args(["--train_dataset", "TOY_train", "--valid_dataset", "TOY_val", "--test_dataset", "TOY_test",
                         "--neigh_epoch_num", "1", "--gossip_epoch_num", "2", "--neigh_tune_lr", "--gossip_tune_lr",
                         "--neigh_batch_size", "64", "--gossip_batch_size", "4",
                         "--neigh_model_path", str(tmp_path / "ckpt_n"), "--gossip_model_path",
                         str(tmp_path / "ckpt_g"), "--train_neigh", "--train_gossip", "--test_gossip",
                         "--output_dir", str(tmp_path / "out")])
    an, ag, ao = config.split_namespaces(args)
    rep = driver.main(an, ag, ao, train_neighborhood=True, train_gossip=True, test_gossip=True,
                      atlas_query_ids=STANDARD_QUERY_IDS, output_dir=str(tmp_path / "out"), data_root=root)
    assert all(np.isfinite(rep["graphlet_mae_gossip"])) and all(np.isfinite(rep["graphlet_mae_neighborhood"]))
    text = (tmp_path / "out" / "config_TOY_test.txt").read_text()
    rates = [float(v) for v in re.findall(r"\blr=([0-9.eE+-]+)", text)]
    print(f"[tuner] main.py: rates in config_TOY_test.txt {rates}")
    assert len(rates) == 2 and rates[0] != 1e-4 and rates[1] != 1e-3
    for rate, d in zip(rates, ("ckpt_n", "ckpt_g")):
        rows = list(csv.reader(open(tmp_path / d / "lr_find.csv")))
        assert 12 < len(rows) <= 101
        assert rate in [float(r[1]) for r in rows[1:]] and 1e-8 <= rate <= 1.0
        assert load_checkpoint(str(tmp_path / d / "last.ckpt"))["hyper_parameters"]["args"].lr == rate
