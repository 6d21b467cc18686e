"""Learning-rate range test: what ``pl.Trainer(auto_lr_find=True).tune(model, datamodule)`` runs before ``fit`` in the
reference's main.py (205-240 neighborhood stage, 338-354 gossip stage; flags ``--neigh_tune_lr`` / ``--gossip_tune_lr``).

The sweep trains for ``num_training`` steps on the native training step (the eager single-process loop of
``Trainer.fit``: forward, ``autograd.backward``, ``optim.Adam.step``) while the rate climbs from ``min_lr`` to
``max_lr``, records the loss per step, and suggests the rate at which the smoothed loss fell fastest.  Afterwards the
model, the dropout stream and the rate are exactly what they were: parameters, ``ops.rng_state`` and ``model.lr`` are
snapshotted first and restored in a ``finally``.

Pinning status: RESTATED, NOT PINNED.  The schedule (``sweep_lrs``), the smoothing and early-stop rule
(``smooth_and_stop``) and the suggestion (``suggest``) restate pytorch_lightning 1.6.4's ``tuner/lr_finder.py``
(``_ExponentialLR`` / ``_LinearLR``, ``_LRCallback.on_train_batch_end``, ``_LRFinder.suggestion``) from its published
source.  Lightning is not installed where this package is built and tested, so no vector produced by Lightning's own
code pins them; ``tests/test_tuner_host.py`` checks them against the formulas written out.  One rule is this package's
own: a non-finite loss ends the sweep (Lightning carries the NaN through every later smoothed value).

Everything above ``lr_find`` is pure numpy / Python floats and importable without a GPU.
"""
from __future__ import annotations

import csv
import math
import warnings
from typing import List, Optional, Sequence, Tuple

import numpy as np


def sweep_lrs(min_lr: float, max_lr: float, num_training: int, mode: str = "exponential") -> List[float]:
    """The rate of every step of the sweep.  Step 0 runs at ``min_lr``; step k >= 1 at ``r = (k + 1) / num_training`` of
    the way to ``max_lr`` (geometrically for "exponential", arithmetically for "linear"), so the last step runs at
    exactly ``max_lr``.  (Lightning 1.6.4 ``_ExponentialLR.get_lr`` / ``_LinearLR.get_lr``: ``curr_iter =
    last_epoch + 1``, and the base rate while ``last_epoch == 0``.  Restated, not pinned: see the module docstring.)"""
    if mode not in ("exponential", "linear"):
        raise ValueError(f"mode must be 'exponential' or 'linear', got {mode!r}")
    if num_training < 1:
        raise ValueError("num_training must be at least 1")
    if not (0.0 < min_lr < max_lr):
        raise ValueError(f"need 0 < min_lr < max_lr, got {min_lr} and {max_lr}")
    min_lr, max_lr = float(min_lr), float(max_lr)
    out = [min_lr]
    for k in range(1, num_training):
        if k == num_training - 1:         # r = 1: max_lr itself, not min_lr * (max_lr / min_lr) one rounding away from it
            out.append(max_lr)
            continue
        r = (k + 1) / num_training
        out.append(min_lr * (max_lr / min_lr) ** r if mode == "exponential" else min_lr + r * (max_lr - min_lr))
    return out


class _Smoother:
    """The running state of ``smooth_and_stop``: feed one raw loss per step."""

    def __init__(self, beta: float = 0.98, early_stop_threshold: Optional[float] = 4.0):
        self.beta, self.threshold = float(beta), early_stop_threshold
        self.avg, self.best, self.k = 0.0, math.inf, 0

    def update(self, raw: float) -> Tuple[float, bool]:
        """(smoothed loss of this step, whether the sweep stops after it)"""
        raw, k = float(raw), self.k
        self.k += 1
        if not math.isfinite(raw):
            return raw, True
        self.avg = self.beta * self.avg + (1.0 - self.beta) * raw
        smoothed = self.avg / (1.0 - self.beta ** (k + 1))
        stop = self.threshold is not None and k > 1 and smoothed > self.threshold * self.best
        if smoothed < self.best or k == 1:
            self.best = smoothed
        return smoothed, stop


def smooth_and_stop(raw_losses: Sequence[float], beta: float = 0.98,
                    early_stop_threshold: Optional[float] = 4.0) -> Tuple[np.ndarray, int]:
    """``(smoothed, n_kept)``: the bias-corrected exponential average of the first ``n_kept`` raw losses, float64, and how
    many steps the sweep runs before the early-stop rule ends it (the step that trips the rule is kept).

        avg_k = beta avg_{k-1} + (1 - beta) raw_k   (avg_{-1} = 0),      smoothed_k = avg_k / (1 - beta^(k+1))

    The sweep stops after step k when k > 1 and smoothed_k > early_stop_threshold * best; ``best`` is updated after
    that check, when smoothed_k < best or k == 1 (so the loss of step 0 never serves as the yardstick).  A non-finite raw
    loss stops the sweep at its step, whose smoothed value is that loss.  ``early_stop_threshold=None`` never stops on a
    finite loss.  (Lightning 1.6.4 ``_LRCallback.on_train_batch_end``; restated, not pinned.)"""
    sm = _Smoother(beta, early_stop_threshold)
    out = []
    for raw in raw_losses:
        s, stop = sm.update(raw)
        out.append(s)
        if stop:
            break
    return np.asarray(out, dtype=np.float64), len(out)


def suggest(lrs: Sequence[float], smoothed: Sequence[float], skip_begin: int = 10, skip_end: int = 1) -> Optional[float]:
    """The rate at the steepest descent of the smoothed loss: drop the first ``skip_begin`` and the last ``skip_end``
    points, then the non-finite ones, and return ``lrs[argmin(np.gradient(loss)) + skip_begin]``; ``None`` with fewer
    than two usable points.  (Lightning 1.6.4 ``_LRFinder.suggestion``; restated, not pinned.)"""
    loss = np.asarray(smoothed, dtype=np.float64)
    loss = loss[skip_begin:max(len(loss) - skip_end, skip_begin)]
    loss = loss[np.isfinite(loss)]
    if loss.size < 2:
        return None
    return float(lrs[int(np.argmin(np.gradient(loss))) + skip_begin])


class LRFinderResult:
    """The record of one sweep.  ``results = {"lr": [...], "loss": [...]}`` as Lightning's ``_LRFinder.results``: the
    rate and the SMOOTHED loss of every step that ran; ``raw_loss`` the losses as the training step returned them."""

    def __init__(self, lrs: Sequence[float], raw_loss: Sequence[float], loss: Sequence[float], stopped_early: bool):
        assert len(lrs) == len(raw_loss) == len(loss)
        self.results = {"lr": [float(v) for v in lrs], "loss": [float(v) for v in loss]}
        self.raw_loss = [float(v) for v in raw_loss]
        self.stopped_early = bool(stopped_early)

    def suggestion(self, skip_begin: int = 10, skip_end: int = 1) -> Optional[float]:
        return suggest(self.results["lr"], self.results["loss"], skip_begin, skip_end)

    def to_csv(self, path: str) -> None:
        with open(path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["step", "lr", "raw_loss", "loss"])
            for k, row in enumerate(zip(self.results["lr"], self.raw_loss, self.results["loss"])):
                w.writerow([k] + [repr(v) for v in row])


def apply_lr(model, lr: Optional[float], flag: str = "auto_lr_find") -> None:
    """``model.lr = lr``, and the ``lr`` of the argparse Namespace the model was built from (``model.args`` / the
    checkpoint's hyper-parameters -- main.py writes the same object to ``config_<dataset>.txt``), so that what is
    recorded is the rate that was used.  ``None`` (the sweep was too short for a suggestion): warn, change nothing."""
    if lr is None:
        warnings.warn(f"{flag}: the sweep kept too few points for a suggestion; the learning rate stays {model.lr}")
        return
    model.lr = float(lr)
    for ns in (getattr(model, "args", None), getattr(model, "hparams_dict", {}).get("args")):
        if ns is not None and hasattr(ns, "lr"):
            ns.lr = float(lr)


def lr_find(trainer, model, datamodule, min_lr: float = 1e-8, max_lr: float = 1.0, num_training: int = 100,
            mode: str = "exponential", early_stop_threshold: Optional[float] = 4.0, update_attr: bool = False,
            skip_begin: int = 10, skip_end: int = 1) -> LRFinderResult:
    """Sweep the learning rate over ``num_training`` eager training steps of ``model`` (always eager, also under
    ``Trainer(graph_capture=True)``: ``optim.Adam.step`` copies each new rate to the device scalar its launch reads) and
    return the record.  Batches come from ``datamodule.train_dataloader()`` in order, wrapping round.  The parameters, the
    dropout stream ``ops.rng_state``, ``model.training`` and ``model.lr`` are restored afterwards, whatever happened;
    with ``update_attr`` the suggestion (``skip_begin`` / ``skip_end`` as in ``suggest``) then becomes the model's rate."""
    import torch
    from . import autograd as AG, ops
    lrs = sweep_lrs(min_lr, max_lr, num_training, mode)
    device = trainer.device
    AG.set_precision(trainer.precision)
    model.to(device)
    params = list(model.parameters())
    rng = ops.rng_state(device)
    saved = [p.detach().clone() for p in params]
    saved_grads = [p.grad for p in params]
    saved_rng, was_training, lr0 = rng.clone(), model.training, model.lr
    raw: List[float] = []
    smoothed: List[float] = []
    stopped = False
    opt = loss = None
    try:
        model.train()
        opt = model.configure_optimizers()["optimizer"]        # (its ReduceLROnPlateau has no part in a sweep)
        sm = _Smoother(0.98, early_stop_threshold)
        stream, batches = iter(datamodule.train_dataloader()), []
        for k, lr in enumerate(lrs):
            batch = None
            if stream is not None:
                try:
                    batch = next(stream).to(device)
                    batches.append(batch)
                except StopIteration:
                    stream = None
            if batch is None:
                if not batches:
                    raise ValueError("lr_find: the training dataloader is empty")
                batch = batches[k % len(batches)]
            i = k if stream is not None else k % len(batches)
            for group in opt.param_groups:
                group["lr"] = lr
            opt.zero_grad(set_to_none=True)
            loss = model.training_step(batch, i)
            AG.backward(loss)
            opt.step()
            raw.append(float(loss.detach()))
            s, stop = sm.update(raw[-1])
            smoothed.append(s)
            if stop:
                stopped = k + 1 < len(lrs)
                break
    finally:
        del opt, loss
        with torch.no_grad():
            for p, s, g in zip(params, saved, saved_grads):
                p.copy_(s)
                p.grad = g
            rng.copy_(saved_rng)
        model.invalidate_caches()
        model.train(was_training)
        model.lr = lr0
    result = LRFinderResult(lrs[:len(raw)], raw, smoothed, stopped)
    if update_attr:
        apply_lr(model, result.suggestion(skip_begin, skip_end))
    return result
