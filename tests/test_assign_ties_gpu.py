"""Exact ties between distinct centroids on lattice palettes: the N-D assign's labels against the
CPU restatement of kd-tree.ts (oracle/), bit for bit.

The inputs (assign_tie_cases.py) make thousands of points sit at exactly the same f64 distance
from 2 to 4,096 centroids, so the label is whichever centroid KdTree.findNearest meets first
(kd-tree.ts:39-68).  That exercises the device tree build (stable order among equal coordinates,
segments of any length), the walk's strict comparisons, the hash-dedup and precomputed-distance
branches of the tie walk, the fix-ups that raise the ties (one tile-half, two halves, the
candidate lists of 64 and 2,048 and their overflow) and the coinciding-centroid descent.
test_assign_ties_cpu.py checks each case's preconditions without a GPU."""
import numpy as np
import pytest

import assign_tie_cases as tc
import oracle
import splat_hip as sh
from test_assign_ties_cpu import oracle_labels
from test_oracle_golden import same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    import torch  # noqa: F401  (torch's HIP runtime first: see splat_hip.Context)
    c = sh.Context(0)
    c.set_profiling(True)
    yield c
    c.set_profiling(False)
    c.close()


def compare(case, got, want, st):
    """labels bit for bit; a mismatch reports how many wrong labels are not even an exact f64
    argmin (a sweep / fix-up error) as opposed to another minimiser (a tie-break error)"""
    got = np.asarray(got, np.uint32)
    bad = got != want
    if bad.any():
        far = tc.not_argmin(case, got, st)
        first = np.nonzero(bad)[0][:5]
        pytest.fail(f'{case.name}: {int(bad.sum())} of {case.n} labels differ from the reference; {far} are not an '
                    f'exact argmin, {int(bad.sum()) - far} are another minimiser (tie-break); '
                    f'{int((bad & ~st["tied"]).sum())} of them at points without a tie; first points {first.tolist()} '
                    f'got {got[first].tolist()} want {want[first].tolist()} multiplicity {st["mult"][first].tolist()}')


@pytest.mark.parametrize('name', tc.NAMES)
def test_assign_exact_ties_vs_oracle(ctx, name, monkeypatch):
    import torch
    dev = torch.device('cuda', 0)
    case, st = tc.build(name), tc.stats(name)
    tc.check_preconditions(case, st)
    want = oracle_labels(case)
    for k_, v in case.env.items():
        monkeypatch.setenv(k_, v)
    ctx.reset_kernel_stats()
    if case.loop:
        cent, got, used = ctx.kmeans(case.cols, case.k, 1, case.draws)
        rc, ocent, _, oused = oracle.kmeans(case.cols, case.k, 1, case.draws)
        assert rc == 0 and used == oused
        ks = ctx.kmeans_stats()
        print(f'{name}: k-means statistics {ks}')
        assert ks['ties'] >= st['ntied'] and ks['pairs'] + ks['ambiguous'] > 0
        # a point's candidate list holds every exact minimiser: more of them than a list has slots
        # is an overflow of the first list (64) and of the second (2,048: the point is walked)
        assert ks['overflow'] >= int((st['mult'] > 64).sum())
        assert ks['walked_overflow'] >= int((st['mult'] > 2048).sum())
    else:
        tcols = [torch.from_numpy(c.copy()).to(dev) for c in case.cols]
        tcen = torch.from_numpy(case.cen.reshape(-1).copy()).to(dev)
        lab = torch.full((case.n,), -1, dtype=torch.int32, device=dev)
        ctx.dev_kmeans_prepare(tcols)
        ctx.dev_kmeans_assign(tcols, case.k, tcen, lab)
        ctx.synchronize()
        got = lab.cpu().numpy().view(np.uint32)
    ties, exact = ctx.kernel_stats('kn.ties')[1], ctx.kernel_stats('kn.exact')[1]
    print(f"{name}: tied={st['ntied']} (listed for the walk {st['walk_tied']}, distinct rows {st['walk_distinct']}) "
          f"largest multiplicity={st['max_mult']} walk={tc.walk_branch(st)} launches kn.ties={ties} kn.exact={exact} "
          f"kn.groups={ctx.kernel_stats('kn.groups')[1]}")
    compare(case, got, want, st)
    if case.loop:  # the update behind the assign (the fused fix-up's sums at this row width)
        same_bits(cent, ocent)
    # the library's own counters around the one assign: the tie walk ran once, and in the wide
    # cases the first candidate lists overflowed (k_exact ran again for the second collect)
    assert ties == 1
    assert exact >= case.min_exact
