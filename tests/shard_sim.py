"""Ranks of the sharded fusion simulated in one process: one thread per rank and an in-process
communicator standing in for pf_dist.TorchComm (all-reduce, point-to-point exchange, broadcast,
agree).  On the GPU every rank has its own panofuse context on the same device; on the CPU the
per-rank compute is the oracle's (tests/test_dist.py's backends) and nothing is synchronised.

A mismatch between the ranks ends as a failed test, not as a wait: the barrier has a timeout, a
failing rank aborts it (and wakes the ranks waiting in agree), and the main thread joins with a
limit.
"""
import threading

import torch


def _sync():
    # a rank's tensors are complete before another thread's stream reads them
    if torch.cuda.is_available():
        torch.cuda.current_stream().synchronize()


class ThreadComm:
    """In-process stand-in for pf_dist.TorchComm among `world` threads."""

    def __init__(self, world):
        self.world = world
        self.bar = threading.Barrier(world, timeout=120)
        self.box = {}
        self.cond = threading.Condition()
        self.aborted = False

    def abort(self):
        """A rank failed: the ranks waiting at the barrier or in agree fail too."""
        with self.cond:
            self.aborted = True
            self.cond.notify_all()
        self.bar.abort()

    def rank(self, r):
        outer = self

        class RankComm:
            nagree = 0

            def all_reduce_sum(self, t):
                outer.box[("ar", r)] = t
                _sync()
                outer.bar.wait()
                if r == 0:
                    acc = outer.box[("ar", 0)].clone()
                    for k in range(1, outer.world):
                        acc += outer.box[("ar", k)]
                    outer.box["ar"] = acc
                _sync()
                outer.bar.wait()
                t.copy_(outer.box["ar"])
                _sync()
                outer.bar.wait()

            def reduce_sum(self, t, dst):
                self.all_reduce_sum(t)

            def exchange(self, sends, recvs):
                # several messages per pair arrive in the order they were sent (as batched
                # isend/irecv pairs match); the clones are complete before another thread's
                # stream reads them (a rank may exchange on its side stream)
                for peer, t in sends:
                    outer.box.setdefault(("x", r, peer), []).append(t.clone())
                _sync()
                outer.bar.wait()
                for peer, t in recvs:
                    t.copy_(outer.box[("x", peer, r)].pop(0))
                outer.bar.wait()

            def broadcast(self, t, src):
                if r == src:
                    outer.box["bc"] = t.clone()
                _sync()
                outer.bar.wait()
                if r != src:
                    t.copy_(outer.box["bc"])
                outer.bar.wait()

            def agree(self, values, src=0, device=None):
                # rank src's list on every rank.  src publishes its k-th list and never waits;
                # the others wait for that list alone, so ranks that all raise the same error
                # from agreed values (a refusal before any exchange) each see it as their own
                key = ("agree", self.nagree)
                self.nagree += 1
                with outer.cond:
                    if r == src:
                        outer.box[key] = [int(v) for v in values]
                        outer.cond.notify_all()
                    while key not in outer.box:
                        if outer.aborted or not outer.cond.wait(120):
                            raise threading.BrokenBarrierError("agree: rank %d gave no list" % src)
                    return list(outer.box[key])

        return RankComm()


def run_ranks(world, body, limit=300):
    """body(rank, comm) on one thread per rank, comm = that rank's end of one ThreadComm.
    Returns (results, errors) per rank, errors[r] = the exception rank r ended with or None; a
    rank still running after `limit` seconds fails the test."""
    comm = ThreadComm(world)
    outs, errs = [None] * world, [None] * world

    def rank_main(r):
        try:
            outs[r] = body(r, comm.rank(r))
        except BaseException as e:  # surfaced by the main thread
            errs[r] = e
            comm.abort()

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(limit)
    assert not any(t.is_alive() for t in th), "a rank is still running"
    return outs, errs
