"""The sharded update's step API on one 1-D column, driven directly in one process (no
process group): st_dev_kmeans_assign / _partials / _finish / _seqsum against the CPU
stand-in's partials / finish / seqsum (tests/dist_oracle_ops.py) on the same labels.

k = 257 is the smallest k whose partials take the radix member order with the values as
payload (k_seg_keys, radix sort, partials1d); k = 256 takes the per-segment counting sort
(seg_label_sort1d) through the same calls.  The column is a normal one with 2% of its values
scaled by 1e-9: the clusters around 0 hold members over many binades, so their sums miss the
certificate and are handed from segment to segment as pending pairs."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'splat-transform_amd', 'py'), os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

NSEG, SEG_LEN = 3, 1399  # three equal segments, no multiple of a tile or a wave


@functools.lru_cache(maxsize=None)
def _column():
    n = NSEG * SEG_LEN
    rng = np.random.default_rng(29)
    v = rng.normal(0, 1, n)
    v = np.where(rng.random(n) < 0.02, v * 1e-9, v).astype(np.float32)
    v.setflags(write=False)
    return v


def _centroids(k):
    return np.linspace(-3.0, 3.0, k).astype(np.float32).reshape(1, k)


def _certified(sabs, emin):
    """the order-free certificate (st_kmeans.h sum_is_exact), elementwise (an empty range's
    exponent, 2^20, is clamped: its sum|x| is 0)"""
    return (sabs == 0.0) | (sabs * (1.0 + 1.0e-6) < np.ldexp(1.0, np.minimum(emin.astype(np.int64), 900) + 53))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize('k', [257, 256])
def test_dist_steps_1d_match_oracle_ops(k):
    import splat_hip as sh
    from dist_oracle_ops import OracleOps
    v = _column()
    n = v.shape[0]
    dev = torch.device('cuda', 0)
    ctx = sh.Context(0)
    ctx.bind_torch_stream(dev)  # before the inputs are made: they are ordered on the same stream
    col = torch.from_numpy(v.copy()).to(dev)
    cen = torch.from_numpy(_centroids(k)).to(dev)
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    ctx.dev_kmeans_assign([col], k, cen, labels)
    sums = torch.empty((NSEG, 1, k), dtype=torch.float64, device=dev)
    sabs = torch.empty((NSEG, 1, k), dtype=torch.float64, device=dev)
    emin = torch.empty((NSEG, 1, k), dtype=torch.int32, device=dev)
    counts = torch.empty((NSEG, k), dtype=torch.int32, device=dev)
    ctx.dev_kmeans_partials([col], NSEG, k, labels, sums, sabs, emin, counts)
    torch.cuda.synchronize()

    # the stand-in's partials on the device's labels
    ref = OracleOps()
    lab = labels.cpu()
    assert int(lab.min()) >= 0 and int(lab.max()) < k
    rs, ra, re, rc = [t.numpy() for t in ref.partials([torch.from_numpy(v.copy())], NSEG, k, lab)]
    # at least one cluster with two or more members in every segment
    assert (rc >= 2).all(axis=0).any()
    assert np.array_equal(counts.cpu().numpy(), rc)
    assert np.array_equal(emin.cpu().numpy(), re)
    ok = _certified(ra, re)  # per (segment, cluster)
    assert ok.any() and not ok.all()
    assert np.array_equal(_bits(sums.cpu().numpy())[ok], _bits(rs)[ok])
    assert np.array_equal(_bits(sabs.cpu().numpy())[ok], _bits(ra)[ok])

    # the fold over the segments (splat_dist.kmeans), each side from its own partials
    S, A, E = sums.sum(0), sabs.sum(0), emin.min(0).values.contiguous()
    C = counts.sum(0, dtype=torch.int32)
    pending = torch.empty(k, dtype=torch.int32, device=dev)
    npend = ctx.dev_kmeans_finish(1, k, S, A, E, C, cen, pending)
    pending = pending[:npend]
    rS, rA, rE, rC = rs.sum(0), ra.sum(0), re.min(0), rc.sum(0)
    rcen = torch.from_numpy(_centroids(k))
    rpend = ref.finish(1, k, torch.from_numpy(rS), torch.from_numpy(rA), torch.from_numpy(rE), torch.from_numpy(rC),
                       rcen)
    assert rpend.numel() >= 1  # at least one pending pair
    assert pending.cpu().tolist() == rpend.tolist()
    done = np.ones(k, bool)
    done[rpend.numpy()] = False
    assert np.array_equal(cen.cpu().numpy().view(np.uint32)[0, done], rcen.numpy().view(np.uint32)[0, done])

    # the pending pairs' running sums, handed from segment to segment in order
    running = torch.zeros(npend, dtype=torch.float64, device=dev)
    rrun = torch.zeros(npend, dtype=torch.float64)
    for seg in range(NSEG):
        ctx.dev_kmeans_seqsum(1, k, seg, pending, running, E, A)
        ref.seqsum(1, k, seg, rpend, rrun)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(running.cpu().numpy()), _bits(rrun.numpy())), seg
    ctx.close()
