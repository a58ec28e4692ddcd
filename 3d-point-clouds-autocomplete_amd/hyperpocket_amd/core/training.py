"""Epoch loops over a device-resident dataset (datasets/device_dataset.py): what core/epoch_loops.py of the reference
computes, with the batches cut on the GPU and the loss terms kept there until the epoch ends."""
import torch

from .._lib import HipExtensionError
from ..losses.champfer_loss import ChamferLoss

_TERMS = ("loss_all", "loss_r", "loss_kld", "loss_emd")


def train_epoch(epoch, engine, batcher):
    """One epoch of engine.step over the batcher's batches.  Returns {'loss_all', 'loss_r', 'loss_kld' [, 'loss_emd']}: the
    mean over the batches of each term (core/epoch_loops.py:41-43), as floats — the terms stay on the device during the
    epoch and come to the host in one transfer at its end.  A term the model does not have is 0.  Raises HipExtensionError
    afterwards if the batcher could not slice some item (its fallback batch was trained on)."""
    steps = [engine.step(existing, missing, gt, epoch) for existing, missing, gt, _ in batcher]
    means = {k: 0.0 for k in _TERMS[:3]}
    if steps:
        names = [k for k in _TERMS if k in steps[0]]
        table = torch.stack([s[k] for s in steps for k in names]).view(len(steps), len(names))
        for k, v in zip(names, table.double().mean(0).tolist()):          # the epoch's one host transfer
            means[k] = v
    failed = batcher.failures()
    if failed:
        raise HipExtensionError(f"epoch {epoch}: no slicing plane was accepted for {failed} item(s) — they were trained on as "
                                "first-`target` points / rest (a degenerate cloud, or max_candidates too small)")
    return means


def val_epoch(epoch, model, batchers_by_category, loss_coef=0.05):
    """The validation numbers of core/epoch_loops.py:49-83: per category the mean over its batches of
    mean(loss_coef * ChamferLoss()(gt, reconstruction)), and 'total', the mean of the categories.  Eval mode, no_grad, one
    host transfer per category; the model's training flag is restored."""
    was_training = model.training
    model.eval()
    chamfer = ChamferLoss()
    losses = {}
    try:
        with torch.no_grad():
            for name, batcher in batchers_by_category.items():
                terms = []
                for existing, missing, gt, _ in batcher:
                    # forward() transposes its inputs in place: hand it views
                    rec = model(existing.view(existing.shape), missing.view(missing.shape), list(gt.shape), epoch, gt.device)
                    terms.append(torch.mean(loss_coef * chamfer(gt, rec.permute(0, 2, 1))))
                if not terms:
                    raise ValueError(f"category {name!r} yields no batch")
                losses[name] = float(torch.stack(terms).double().mean().item())
    finally:
        model.train(was_training)
    losses["total"] = sum(losses.values()) / len(losses) if losses else 0.0
    return losses
