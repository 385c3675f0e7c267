"""Ranks of a tensor-parallel group as threads of ONE process on one GPU (tests/test_gpu_tp.py)."""
import threading

import torch


class LockstepGroup:
    """Two (or more) ranks of ONE process, one thread each, sharing the GPU's default stream: all_gather = everybody
    publishes its slice, meets at a barrier, copies all slices (stream order makes them ready), meets again (nobody
    overwrites a slice somebody still has to copy).  Stands in for the process group so that the P > 1 launch sequence
    of the decode engine -- shard offsets, slice reassembly, residual slices -- runs on a one-GPU box."""

    def __init__(self, world):
        self.world = world
        self.slots = [None] * world
        self.barrier = threading.Barrier(world)

    def view(self, rank):
        parent = self

        class _Rank:
            world, slots, barrier = parent.world, parent.slots, parent.barrier

            def __init__(self):
                self.rank = rank

            def all_gather(self, out, inp):
                self.slots[self.rank] = inp
                self.barrier.wait()
                out.view(self.world, -1).copy_(torch.stack([t.reshape(-1) for t in self.slots]))
                self.barrier.wait()

            def all_reduce(self, t):
                self.slots[self.rank] = t
                self.barrier.wait()
                total = torch.stack(list(self.slots)).sum(0)     # the same reduction on every rank
                self.barrier.wait()                              # everybody has read every slot
                t.copy_(total)
        return _Rank()


def run_ranks(group, dev, fn, timeout=120):
    """fn(rank) on one thread per rank; a rank that raises aborts the barrier, so the others leave it instead of waiting for a
    peer that never comes.  Returns (results per rank, exceptions)."""
    outs, errs = [None] * group.world, []

    def run(r):
        try:
            torch.cuda.set_device(dev)
            outs[r] = fn(r)
        except Exception as e:       # noqa: BLE001 -- a dead rank must not leave the others at the barrier
            errs.append(e)
            group.barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(group.world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=timeout)
    return outs, errs
