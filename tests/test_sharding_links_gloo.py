"""The link spheres through the sharding layer on the CPU: world-size-2 gloo processes shard a batch whose arms are each other's obstacles.
ShardedEngine.link_points_host and set_coupling take `src_arm` in GLOBAL arm indices and translate it per shard; a source that lies in
another shard is refused with ValueError (there is no plumbing between handles).  The stand-in engine computes the points on the host
(tests/hp_links.py: host_points) -- the product has no CPU path."""
import os
import socket
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hp_links as hl  # noqa: E402

SPHERES = [(6, (0.01, 0.0, 0.02), 0.06), (2, (0.0, 0.03, 0.0), 0.05), (7, (0.0, 0.0, 0.0), 0.07)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _LinkEngine:
    """Stand-in for engine.Engine: the link-sphere surface alone, the points from the host's float64 walk."""
    io_dtype = np.dtype(np.float64)

    def __init__(self, chain, batch, device=0, **kw):
        self.chain, self.batch, self.device = chain, batch, device
        self.spheres, self.coupling = [], None

    def set_link_spheres(self, spheres):
        self.spheres = list(spheres or ())

    def link_points_host(self, q, src_arm=None, xform=None, out=None, n_rep=None, first_rep=0):
        assert q.shape[0] == self.batch and (src_arm is None or (src_arm.shape == (self.batch,) and src_arm.max() < self.batch))
        L = len(self.spheres)
        n_rep = first_rep + L if n_rep is None else n_rep
        out = np.full((self.batch, n_rep, 4), np.nan)
        out[:, first_rep:first_rep + L] = hl.host_points(self.chain, self.spheres, q, src_arm, xform)
        return out

    def set_coupling(self, src_arm=None, xform=None, first_rep=0, link_traj=None, trace_checks=None):
        self.coupling = None if src_arm is None and xform is None and trace_checks is None else (src_arm, xform, first_rep, trace_checks)

    def close(self):
        pass


def _case(batch):
    chain = hl.chain_of("lwr")
    q, x = hl.inputs(chain, batch, np.float64, seed=23)
    return chain, q, x


def _worker(rank, world, port, batch, q_out):
    import torch
    import torch.distributed as dist
    from vfclik_amd import sharding
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    chain, q, x = _case(batch)
    sh = sharding.ShardedEngine(chain, batch, devices=[0], engine_factory=_LinkEngine)
    sh.set_link_spheres(SPHERES)
    pair = np.arange(batch, dtype=np.int32) ^ 1
    pair[pair >= batch] = -1
    refused = None
    try:
        rows = sh.link_points_host(q, pair, x, n_rep=5, first_rep=1)
        sh.set_coupling(src_arm=pair, xform=x, first_rep=1)
        a, b, e = sh.parts[0]
        want = np.where(pair[a:b] >= 0, pair[a:b] - a, -1)
        assert np.array_equal(e.coupling[0], want) and np.array_equal(e.coupling[1], x[a:b]) and e.coupling[2] == 1
        sh.set_coupling(None)
        assert e.coupling is None
        full = sh.gather(torch.from_numpy(rows)).numpy()
    except ValueError as err:
        refused, full = str(err), None
    # a source of its own shard, given in this rank's rows
    own = sh.link_points_host(sh.local(q), np.full(sh.local_rows, sh.lo, dtype=np.int32), None, global_rows=False)
    assert own.shape == (sh.local_rows, 3, 4) and np.all(own == own[0])
    ok = torch.tensor([0.0 if refused else 1.0])
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)      # (every rank leaves the collective path together)
    q_out.put((rank, refused, full))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("batch,crossing", [(64, False), (101, True), (102, True)])
def test_two_ranks_sources_in_global_indices(batch, crossing):
    """64 arms: 32 + 32, every pair inside a shard -- the collated rows are the un-sharded ones.  101 arms: 51 + 50, the pair (50, 51)
    straddles the cut, both ranks refuse.  102 arms: 51 + 51, likewise."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q_out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, batch, q_out)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict((r, (refused, full)) for r, refused, full in (q_out.get(timeout=120) for _ in range(2)))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    if crossing:
        for r in range(2):
            assert got[r][0] is not None and "another shard" in got[r][0], got[r][0]
        return
    chain, q, x = _case(batch)
    pair = np.arange(batch) ^ 1
    ref = np.full((batch, 5, 4), np.nan)
    ref[:, 1:4] = hl.host_points(chain, SPHERES, q, pair, x)
    for r in range(2):
        assert got[r][0] is None and np.array_equal(got[r][1], ref, equal_nan=True)


def test_single_process_parts_translate_and_refuse():
    from vfclik_amd import sharding
    chain, q, x = _case(12)
    sh = sharding.ShardedEngine(chain, 12, rank=0, world=1, devices=[0, 1, 2], engine_factory=_LinkEngine)   # parts of 4 arms
    sh.set_link_spheres(SPHERES)
    pair = np.arange(12, dtype=np.int32) ^ 1
    rows = sh.link_points_host(q, pair, x)
    assert np.array_equal(rows, hl.host_points(chain, SPHERES, q, pair, x))
    assert np.array_equal(sh.link_points_host(q), hl.host_points(chain, SPHERES, q))   # every arm its own source
    with pytest.raises(ValueError, match="another shard"):
        sh.link_points_host(q, (np.arange(12, dtype=np.int32) + 4) % 12)
    with pytest.raises(ValueError, match="another shard"):
        sh.set_coupling(src_arm=np.zeros(12, dtype=np.int32))
    none = np.full(12, -1, dtype=np.int32)
    sh.set_coupling(src_arm=none, first_rep=2)
    assert all(np.array_equal(e.coupling[0], none[:4]) and e.coupling[2] == 2 for e in sh.engines)
    sh.close()
