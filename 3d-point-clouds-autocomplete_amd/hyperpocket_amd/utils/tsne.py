"""Exact t-SNE on the device (csrc/tsne.hip): squared distances, perplexity calibration and the O(n^2) gradient
iterations as HIP kernels, the rest — the initial embedding, the learning rate — as plumbing in torch.

It stands where the reference's make_tsne_reduction calls scikit-learn's manifold.TSNE(n_components=2, init='pca'): the same
objective, schedule (early exaggeration 12 for 250 iterations at momentum 0.5, then momentum 0.8), gains and 'auto'
learning rate, with three stated differences.  The gradient is exact, not the Barnes-Hut approximation.  There is no
convergence test: all max_iter iterations run, enqueued without a host synchronisation.  And the result is reproducible to
the bit: no float atomics in the kernels, and an initial embedding that draws nothing — scikit-learn's 'pca' runs a
randomised solver under random_state=None.
"""
from collections import namedtuple

import torch

from .. import ops

TsneResult = namedtuple("TsneResult", "embedding kl beta steps")
TsneGradient = namedtuple("TsneGradient", "grad Z kl")


def pairwise_sqdist(X):
    """D (n, n) float32 of the rows of X (n, d): ops.pairwise_sqdist."""
    return ops.pairwise_sqdist(X)


def affinities(D, perplexity):
    """(P, beta, steps) of squared distances D (n, n): ops.tsne_affinities."""
    return ops.tsne_affinities(D, perplexity)


def tsne_gradient(P, Y, exaggeration=1.0, kl=False):
    """The gradient of the t-SNE objective at Y (n, 2) under P (n, n) -> TsneGradient(grad (n, 2), Z, kl): the kernels of one
    descent iteration, with the update applied to scratch copies so that Y stays.  Z and kl are 0-dim device tensors, and
    None unless kl=True, which costs a logarithm per pair."""
    out = torch.zeros(3, dtype=torch.float32, device=Y.device) if kl else None
    rowacc = ops.tsne_gradient_rows(P, Y, exaggeration, kl=out)
    grad = torch.empty_like(Y)
    update, gains, _ = ops.tsne_state(Y)
    ops.tsne_update(rowacc, Y.clone(), update, gains, 0.0, 0.0, grad=grad)
    return TsneGradient(grad, out[1] if kl else None, out[0] if kl else None)


def classical_scaling(D, scale=1e-4):
    """The first two principal-component scores of the rows behind the squared distances D (n, n), by classical scaling: the
    top two eigenpairs (lambda, v) of -1/2 J D J, J = I - 11^T / n, give the scores v sqrt(lambda) — the Gram matrix of the
    centred rows is that matrix, so no second pass over the rows is needed.  Each column is flipped so that its entry of
    largest magnitude is positive, and both are scaled by one factor that brings column 0 to standard deviation `scale`
    (scikit-learn's convention for a PCA start).  float64 inside, any device; returns (n, 2) float32."""
    B = D.to(torch.float64)
    B = B - B.mean(0, keepdim=True)
    B = B - B.mean(1, keepdim=True)
    B = -0.25 * (B + B.t())                              # -1/2 of the symmetric part: symmetric to the bit
    lam, vec = torch.linalg.eigh(B)
    Y = vec[:, [-1, -2]] * lam[[-1, -2]].clamp_min(0).sqrt()
    pick = Y.abs().argmax(0)
    Y = Y * torch.where(Y[pick, torch.arange(2, device=Y.device)] < 0, -1.0, 1.0)
    std = Y[:, 0].std(unbiased=False)
    if float(std) > 0:
        Y = Y / std * scale
    return Y.to(torch.float32).contiguous()


def auto_learning_rate(n, early_exaggeration):
    """scikit-learn's 'auto': max(n / early_exaggeration / 4, 50)."""
    return max(n / early_exaggeration / 4.0, 50.0)


def initial_embedding(init, n, D, seed, device):
    if isinstance(init, torch.Tensor):
        if tuple(init.shape) != (n, 2):
            raise ValueError(f"init must be ({n}, 2), got {tuple(init.shape)}")
        return init.to(device, torch.float32).clone().contiguous()
    if init == 'random':
        g = torch.Generator().manual_seed(int(seed))
        return (1e-4 * torch.randn(n, 2, generator=g, dtype=torch.float32)).to(device)
    if init == 'pca':
        return classical_scaling(D).to(device)
    raise ValueError("init must be 'pca', 'random' or a (n, 2) tensor")


def tsne(X, perplexity=30.0, max_iter=1000, init='pca', early_exaggeration=12.0, explore=250, learning_rate='auto', seed=0):
    """Exact t-SNE of the rows of X (n, d) float32 on the device -> TsneResult(embedding (n, 2) float32, kl — the KL
    divergence of the embedding, a 0-dim device tensor —, beta (n), steps (n): the calibration's precisions and evaluation
    counts).  Iterations below `explore` run under early_exaggeration and momentum 0.5, the others under 1 and 0.8.
    init: 'pca' (classical_scaling of the distances in hand), 'random' (1e-4 times a CPU normal draw under `seed`) or a
    (n, 2) tensor.  Memory: the distances, the conditional and the joint probabilities, n * n floats each."""
    if not isinstance(X, torch.Tensor) or X.dim() != 2:
        raise ValueError("X must be a (n, d) tensor")
    n = X.size(0)
    if not 0.0 < float(perplexity) < n:
        raise ValueError(f"perplexity must be positive and below the number of rows ({n}), got {perplexity}")
    D = ops.pairwise_sqdist(X)
    Y = initial_embedding(init, n, D, seed, X.device)
    P, beta, steps = ops.tsne_affinities(D, perplexity, ws=None)
    del D
    lr = auto_learning_rate(n, early_exaggeration) if learning_rate == 'auto' else float(learning_rate)
    update, gains, rowacc = ops.tsne_state(Y)
    kl = torch.zeros(3, dtype=torch.float32, device=X.device)
    ops.tsne_descend(P, Y, update, gains, rowacc, 0, int(max_iter), int(explore), early_exaggeration, lr, kl=kl)
    return TsneResult(Y, kl[0], beta, steps)
