"""The SyncBatchNorm exchange over a real process group (gloo, two ranks, CPU), in the manner of tests/test_dist.py:
`simpledet_amd.dist.all_gather_stats` stacks the ranks' (2, C) blocks in rank order, and composed with the
contract's arithmetic of tests/sync_bn_ref.py per rank it reproduces batch normalisation over the whole batch."""
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SHAPE, EPS = (6, 5, 4, 3), 1e-3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _case():
    from tests import sync_bn_ref as sr
    return sr.make_case(np.random.RandomState(31), SHAPE, "random", False, 3.0, EPS)


def _rank_part(x):
    """a rank's (2, C) block: mean and biased variance about it (float64 here, rounded once: the statistics
    kernel's accuracy is the GPU tests' subject, the exchange is this one's)"""
    ax = (0,) + tuple(range(2, x.ndim))
    x64 = x.astype(np.float64)
    m = x64.mean(axis=ax)
    v = ((x64 - m.reshape((1, -1) + (1,) * (x.ndim - 2))) ** 2).mean(axis=ax)
    return np.stack([m, v]).astype(F)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    ndev = torch.cuda.device_count()
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank % ndev if ndev else rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from simpledet_amd import dist as sdd
    from tests import sync_bn_ref as sr
    r, _, w = sdd.init("gloo")
    assert (r, w) == (rank, world)
    c = _case()
    x, dy = sr.slices(c["x"], world)[rank], sr.slices(c["dy"], world)[rank]
    part = torch.from_numpy(_rank_part(x))
    parts, got_rank = sdd.all_gather_stats(part)
    assert tuple(parts.shape) == (world, 2, SHAPE[1]) and parts.dtype == torch.float32
    mean, var = sr.combine_contract(parts.numpy())
    y = sr.fwd_contract32(x, mean, var, c["gamma"], c["beta"], EPS, False)
    ax = (0, 2, 3)
    bpart = np.stack([dy.sum(axis=ax, dtype=np.float64),
                      (dy.astype(np.float64) * (x - mean.reshape(1, -1, 1, 1))).sum(axis=ax)]).astype(F)
    bparts, rank2 = sdd.all_gather_stats(torch.from_numpy(bpart))
    b = sr.bwd_contract32(dy, x, mean, var, c["gamma"], bparts.numpy(), rank2, sr.count(x), EPS, False)
    q.put((rank, got_rank, rank2, parts.numpy(), bparts.numpy(), part.numpy(), bpart, mean, var, y, b["dx"],
           b["dgamma"], b["dbeta"]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_gather_in_rank_order_and_reproduce_the_whole_batch():
    from tests import sync_bn_ref as sr
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=120) for _ in range(2)], key=lambda t: t[0])
        for p in procs:
            p.join(60)
            assert p.exitcode == 0
    finally:
        for p in procs:  # a rank left waiting for a failed peer must not outlive the test
            if p.is_alive():
                p.terminate()
                p.join(10)
    (r0, g0, h0, parts0, bparts0, part0, bpart0, mean0, var0, y0, dx0, dg0, db0) = res[0]
    (r1, g1, h1, parts1, bparts1, part1, bpart1, mean1, var1, y1, dx1, dg1, db1) = res[1]
    assert (r0, g0, h0) == (0, 0, 0) and (r1, g1, h1) == (1, 1, 1)             # the rank that comes back
    # the same (2, 2, C) on both ranks, rank order: row r is rank r's own block
    assert np.array_equal(parts0, parts1) and np.array_equal(bparts0, bparts1)
    assert np.array_equal(parts0[0], part0) and np.array_equal(parts0[1], part1)
    assert np.array_equal(bparts0[0], bpart0) and np.array_equal(bparts0[1], bpart1)
    assert np.array_equal(mean0, mean1) and np.array_equal(var0, var1)        # the same bits on every rank
    # ... and the whole batch's normalisation comes out
    c = _case()
    truth, T, k_ref, _, _ = sr.evaluate(c, 2)
    bt, bT = sr.bwd_truth(c["dy"], c["x"], mean0, var0, c["gamma"], EPS, False, 2)
    bref = sr.bwd_ref32(c["dy"], c["x"], mean0, var0, c["gamma"], EPS, False, 2)
    got = dict(mean=mean0, var=var0, y=np.concatenate([y0, y1]))
    for o in ("mean", "var", "y"):
        k = sr.k_of(got[o], truth[o], T[o])
        assert k <= 2 * k_ref[o] + 2, (o, k, k_ref[o])
    gotb = dict(dx=np.concatenate([dx0, dx1]), dgamma=dg0.astype(np.float64) + dg1, dbeta=db0.astype(np.float64) + db1)
    for o in ("dx", "dgamma", "dbeta"):
        k, kr = sr.k_of(gotb[o], bt[o], bT[o]), sr.k_of(bref[o], bt[o], bT[o])
        assert k <= 2 * kr + 2, (o, k, kr)


def test_without_a_process_group_there_is_no_collective():
    from simpledet_amd import dist as sdd
    assert not dist.is_initialized()
    part = torch.arange(10, dtype=torch.float32).reshape(2, 5)
    parts, rank = sdd.all_gather_stats(part)
    assert rank == 0 and tuple(parts.shape) == (1, 2, 5) and torch.equal(parts[0], part)
    assert parts.data_ptr() == part.data_ptr()                                # a view: nothing was copied
