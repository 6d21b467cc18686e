"""The pure half of the learning-rate range test (desco_amd/tuner.py): the schedule, the smoothing and early-stop rule
and the suggestion, each against its formula written out here.  (Restated from Lightning 1.6.4, which is not installed:
nothing here is a vector Lightning produced.)"""
import csv
import math

import numpy as np
import pytest

from desco_amd import tuner


# ---- sweep_lrs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["exponential", "linear"])
@pytest.mark.parametrize("lo,hi,n", [(1e-8, 1.0, 100), (1e-6, 1e-1, 24), (3e-5, 0.7, 7), (1e-4, 1e-2, 2)])
def test_sweep_lrs_ends_and_formula(mode, lo, hi, n):
    lrs = tuner.sweep_lrs(lo, hi, n, mode)
    assert len(lrs) == n and all(isinstance(v, float) for v in lrs)
    assert lrs[0] == lo and lrs[-1] == hi                     # exactly
    want = [lo]
    for k in range(1, n):
        r = (k + 1) / n
        want.append(lo * (hi / lo) ** r if mode == "exponential" else lo + r * (hi - lo))
    np.testing.assert_allclose(lrs, want, rtol=1e-15, atol=0)


def test_sweep_lrs_exponential_ratio_is_constant_from_step_1():
    lrs = np.array(tuner.sweep_lrs(1e-8, 1.0, 100, "exponential"))
    ratio = lrs[2:] / lrs[1:-1]
    np.testing.assert_allclose(ratio, (1.0 / 1e-8) ** (1 / 100), rtol=1e-13)
    assert lrs[1] / lrs[0] == pytest.approx((1.0 / 1e-8) ** (2 / 100), rel=1e-13)     # step 0 -> 1 covers two shares


def test_sweep_lrs_linear_is_equidistant_from_step_1():
    lrs = np.array(tuner.sweep_lrs(1e-4, 1e-1, 50, "linear"))
    np.testing.assert_allclose(np.diff(lrs[1:]), (1e-1 - 1e-4) / 50, rtol=1e-11)
    assert np.all(np.diff(lrs) > 0)


def test_sweep_lrs_single_step_and_bad_arguments():
    assert tuner.sweep_lrs(1e-5, 1e-2, 1) == [1e-5]
    with pytest.raises(ValueError):
        tuner.sweep_lrs(1e-5, 1e-2, 10, "cosine")
    with pytest.raises(ValueError):
        tuner.sweep_lrs(1e-2, 1e-5, 10)
    with pytest.raises(ValueError):
        tuner.sweep_lrs(1e-5, 1e-2, 0)


# ---- smooth_and_stop ------------------------------------------------------------------------------------------------
def _smooth_by_hand(raw, beta):
    avg, out = 0.0, []
    for k, v in enumerate(raw):
        avg = beta * avg + (1 - beta) * v
        out.append(avg / (1 - beta ** (k + 1)))
    return np.array(out)


def test_constant_sequence_smooths_to_itself():
    sm, n = tuner.smooth_and_stop([3.25] * 60)
    assert n == 60 and sm.dtype == np.float64
    np.testing.assert_allclose(sm, 3.25, rtol=1e-12)


def test_smoothing_matches_the_formula():
    rng = np.random.default_rng(0)
    raw = 2.0 + rng.random(80)
    sm, n = tuner.smooth_and_stop(raw, beta=0.9, early_stop_threshold=None)
    assert n == 80
    np.testing.assert_allclose(sm, _smooth_by_hand(raw, 0.9), rtol=1e-13)


def test_jump_at_step_30_stops_there():
    """The rule compares SMOOTHED losses.  With beta = 0 the smoothed loss is the raw one, so a raw jump to 5x at step 30
    is a smoothed jump to 5x > 4x best.  With the default beta = 0.98 a raw jump to 5x moves the smoothed loss to
    (0.98 (1 - 0.98^30) + 0.02 * 5) / (1 - 0.98^31) = 1.17x only and the sweep goes on; a raw jump to 100x moves it to
    5.25x and stops the sweep."""
    raw = [2.0] * 30 + [10.0] + [2.0] * 9
    sm, n = tuner.smooth_and_stop(raw, beta=0.0)
    assert n == 31 and len(sm) == 31 and sm[30] == 10.0
    sm, n = tuner.smooth_and_stop(raw)
    assert n == 40 and sm[30] == pytest.approx(2.0 * (0.98 * (1 - 0.98 ** 30) + 0.1) / (1 - 0.98 ** 31), rel=1e-12)
    raw[30] = 200.0
    sm, n = tuner.smooth_and_stop(raw)
    assert n == 31 and sm[30] > 4 * 2.0
    np.testing.assert_allclose(sm, _smooth_by_hand(raw[:31], 0.98), rtol=1e-13)


def test_jump_at_step_1_does_not_stop():
    """k > 1: the rule is not applied at step 1, whose loss then becomes the yardstick (``or k == 1``)."""
    raw = [2.0, 10.0] + [2.0] * 20
    sm, n = tuner.smooth_and_stop(raw, beta=0.0)
    assert n == 22
    # the same jump one step later does stop
    sm, n = tuner.smooth_and_stop([2.0, 2.0, 10.0] + [2.0] * 20, beta=0.0)
    assert n == 3
    # and step 1 replaces step 0 as the yardstick even when it is worse: 30 < 4 * 10 goes on, 41 stops
    assert tuner.smooth_and_stop([2.0, 10.0, 30.0, 2.0], beta=0.0)[1] == 4
    assert tuner.smooth_and_stop([2.0, 10.0, 41.0, 2.0], beta=0.0)[1] == 3


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("threshold", [4.0, None])
def test_non_finite_loss_stops_at_its_step(bad, threshold):
    raw = [2.0] * 7 + [bad] + [2.0] * 5
    sm, n = tuner.smooth_and_stop(raw, early_stop_threshold=threshold)
    assert n == 8 and len(sm) == 8
    assert not math.isfinite(sm[7]) and np.all(np.isfinite(sm[:7]))


def test_no_threshold_keeps_everything():
    raw = [1.0] * 10 + [1e6] * 10
    sm, n = tuner.smooth_and_stop(raw, early_stop_threshold=None)
    assert n == 20 and len(sm) == 20
    assert tuner.smooth_and_stop(raw)[1] < 20


# ---- suggest --------------------------------------------------------------------------------------------------------
def _v_curve(n=60):
    lrs = tuner.sweep_lrs(1e-6, 1.0, n)
    x = np.arange(n)
    raw = np.where(x < 40, 5.0 - 4.0 / (1 + np.exp(-(x - 25) / 3.0)), 1.0 + 0.4 * (x - 40) ** 2 / 10)
    sm, _ = tuner.smooth_and_stop(raw, beta=0.5, early_stop_threshold=None)
    return lrs, sm


def test_suggest_is_the_steepest_descent_of_a_v_curve():
    lrs, sm = _v_curve()
    got = tuner.suggest(lrs, sm)
    idx = int(np.argmin(np.gradient(np.asarray(sm)[10:-1]))) + 10
    assert got == lrs[idx]
    assert 20 <= idx <= 32                        # on the falling flank (its steepest raw point is step 25), not the rising one
    assert sm[idx + 1] < sm[idx - 1]
    # other windows
    for b, e in ((0, 1), (3, 5), (22, 0)):
        w = np.asarray(sm)[b:len(sm) - e]
        assert tuner.suggest(lrs, sm, skip_begin=b, skip_end=e) == lrs[int(np.argmin(np.gradient(w))) + b]


def test_suggest_needs_two_usable_points():
    lrs = tuner.sweep_lrs(1e-6, 1.0, 12)
    sm = list(np.linspace(3, 1, 12))
    assert tuner.suggest(lrs, sm) is None                     # 12 - 10 - 1 = 1 point
    assert tuner.suggest(lrs[:5], sm[:5]) is None             # none
    assert tuner.suggest(lrs, sm, skip_begin=9) is not None   # 2 points
    assert tuner.suggest(lrs, [float("nan")] * 12, skip_begin=0) is None
    assert tuner.suggest([], []) is None


def test_suggest_ignores_non_finite_entries():
    lrs, sm = _v_curve()
    want = tuner.suggest(lrs, sm)
    tail = np.array(sm, dtype=np.float64)
    tail[50:] = np.inf                     # a diverged tail behind the descent: dropped, the same suggestion
    assert tuner.suggest(lrs, tail) == want
    tail[55] = np.nan
    assert tuner.suggest(lrs, tail) == want


# ---- LRFinderResult -------------------------------------------------------------------------------------------------
def test_result_record_and_csv(tmp_path):
    lrs, sm = _v_curve()
    raw = [v + 0.25 for v in sm]
    res = tuner.LRFinderResult(lrs, raw, sm, stopped_early=False)
    assert res.results["lr"] == lrs and res.results["loss"] == list(sm) and res.raw_loss == raw
    assert res.suggestion() == tuner.suggest(lrs, sm) and res.suggestion(skip_begin=3) == tuner.suggest(lrs, sm, 3, 1)
    assert res.stopped_early is False
    path = tmp_path / "lr_find.csv"
    res.to_csv(str(path))
    rows = list(csv.reader(open(path)))
    assert rows[0] == ["step", "lr", "raw_loss", "loss"] and len(rows) == len(lrs) + 1
    for k, row in enumerate(rows[1:]):
        assert int(row[0]) == k and [float(v) for v in row[1:]] == [lrs[k], raw[k], sm[k]]     # values round-trip exactly


def test_apply_lr_sets_model_and_namespace_or_warns():
    import argparse
    ns = argparse.Namespace(lr=1e-4, dropout=0.0)

    class M:
        pass
    m = M()
    m.lr, m.args, m.hparams_dict = 1e-4, ns, {"args": ns}
    tuner.apply_lr(m, 3e-3)
    assert m.lr == 3e-3 and ns.lr == 3e-3
    with pytest.warns(UserWarning, match="too few points"):
        tuner.apply_lr(m, None)
    assert m.lr == 3e-3 and ns.lr == 3e-3
    g = M()                                   # the gossip model keeps its Namespace in the hyper-parameters only
    g.lr, g.hparams_dict = 1e-3, {"args": argparse.Namespace(lr=1e-3)}
    tuner.apply_lr(g, 2e-2)
    assert g.lr == 2e-2 and g.hparams_dict["args"].lr == 2e-2


# ---- Trainer.tune without a sweep -----------------------------------------------------------------------------------
def test_trainer_names_the_tune_flags_and_tune_bs_only_warns():
    import warnings
    from desco_amd.trainer import Trainer
    tr = Trainer(accelerator="cpu")
    assert tr.auto_lr_find is False and not tr.auto_scale_batch_size
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert tr.tune(object()) == {}
    tr = Trainer(accelerator="cpu", auto_scale_batch_size=True)
    with pytest.warns(UserWarning, match="tune_bs|auto_scale_batch_size"):
        assert tr.tune(object()) == {}
    assert Trainer(accelerator="cpu", auto_lr_find=True).auto_lr_find is True
