"""W ranks of a cell-sharded fit on ONE GPU: W ``HipEngine`` handles (``rank=r, world=W``) on W host threads, joined by the host all-reduce hook of the
C ABI (ca_set_host_allreduce).  Shared by tests/test_gpu_sharding.py and tests/test_gpu_shard_grad.py.

The rig ends on trouble, it never waits: the barrier has a time limit, a worker that raises aborts it (every peer inside a collective then leaves with
CA_ERR_COMM through the hook's return code), the threads are joined with a time limit and a thread still alive fails the test.  Workers only COLLECT
arrays; whoever uses ``run_ranks`` asserts on the main thread after the join, so that a failed comparison cannot leave a peer inside a collective.
"""
import threading

from clonealign_amd.sharding import cell_range

SHARDED_INPUTS = ("Y", "psi0", "X", "extra_loglik")     # the constructor arguments indexed by cell
CELL_VARS = ("psi", "gamma_logits")                     # the variables a rank holds its slice of; every other variable is replicated
COMM_TIMEOUT_MS = 5000


class HostAllreduce:
    """The sum over the ranks' buffers, between threads.  ``sizes``: the length of every collective, as rank 0 saw them."""
    def __init__(self, world, timeout=120.0):
        self.world = world
        self.bar = threading.Barrier(world, timeout=timeout)
        self.slots = [None] * world
        self.sizes = []

    def make(self, rank):
        def fn(buf):
            self.slots[rank] = buf.copy()
            self.bar.wait()
            tot = self.slots[0].copy()
            for r in range(1, self.world):
                tot += self.slots[r]
            self.bar.wait()
            buf[:] = tot
            if rank == 0:
                self.sizes.append(len(buf))
        return fn


def ranges(N, world):
    return [cell_range(N, r, world) for r in range(world)]


def shard_case(case, lo, hi):
    """The constructor arguments of the rank that holds cells [lo, hi)."""
    out = dict(case)
    for k in SHARDED_INPUTS:
        if out.get(k) is not None:
            out[k] = out[k][lo:hi]
    return out


def shard_value(name, value, lo, hi):
    """What a rank ``set``s for variable ``name`` of the whole state: its slice of psi and gamma_logits, everything else whole."""
    return value[lo:hi] if name in CELL_VARS else value


def run_ranks(world, body, join_timeout=120.0, barrier_timeout=60.0):
    """``body(rank, allreduce_hook, ar)`` on ``world`` threads; returns the list of what the bodies returned.  Raises (on the calling thread) if a worker raised
    or did not come back within ``join_timeout`` seconds."""
    ar = HostAllreduce(world, timeout=barrier_timeout)
    out, err = [None] * world, []

    def worker(rank):
        try:
            out[rank] = body(rank, ar.make(rank), ar)
        except BaseException as e:  # noqa: BLE001
            err.append((rank, repr(e)))
            ar.bar.abort()

    ts = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(join_timeout)
    alive = [r for r, t in enumerate(ts) if t.is_alive()]
    if alive:
        ar.bar.abort()
    assert not alive, f"ranks {alive} did not come back within {join_timeout} s"
    assert not err, err
    return out


def sharded_engines(case, world, body, engine_kw=None, **kw):
    """One engine per rank over ``cell_range`` of ``case`` (comm_timeout_ms = 5000), ``body(eng, rank, lo, hi, ar)`` on each, the engines closed whatever happens."""
    from clonealign_amd.engine import HipEngine
    N = case["Y"].shape[0]

    def per_rank(rank, hook, ar):
        lo, hi = cell_range(N, rank, world)
        eng = HipEngine(**shard_case(case, lo, hi), rank=rank, world=world, host_allreduce=hook, comm_timeout_ms=COMM_TIMEOUT_MS, **(engine_kw or {}))
        try:
            return body(eng, rank, lo, hi, ar)
        finally:
            eng.close()

    return run_ranks(world, per_rank, **kw)
