"""Gradient all-reduce over the flat gradient buffer of a trainer (RCCL on the GPUs, gloo in the CPU tests): buckets released while
backward still runs (BucketReducer; cdnet_amd.trainer maps the tape's parameters to flat offsets) or one pass behind it
(bucketed_allreduce)."""


class BucketReducer:
    """Releases buckets of a flat gradient buffer to the all-reduce as soon as they are complete.
    The buffer is laid out in forward order and backward fills it from the end: `pending` maps the start offset of
    every tensor that still waits for its gradient to its end offset; a bucket [a, b) is launched (async all-reduce,
    top-down) once no pending tensor reaches into or above it.  Bucket boundaries are counted from the TOP of the used
    range (n, n - B, n - 2B, ..., 0): the remainder bucket is then the lowest one - the one that completes last, with the
    first layers' gradients at the very end of backward, and whose collective nothing is left to hide (59 MB of
    gradients in 25 MB buckets: a 6 MB tail instead of a 25 MB one).  Every rank runs the same schedule, so the
    collectives are issued in the same order everywhere.  Backend-agnostic (RCCL on the GPUs, gloo in the CPU tests)."""

    def __init__(self, flat, n_used, bucket_elems, pending):
        self.flat, self.n, self.bucket = flat, n_used, bucket_elems
        self.pending = dict(pending)
        self.works = []
        self.bounds = [n_used]                       # descending bucket boundaries
        while self.bounds[-1] > 0:
            self.bounds.append(max(0, self.bounds[-1] - bucket_elems))
        self.next = 0                                # buckets [bounds[j + 1], bounds[j]) with j < next are in flight
        self.early = 0                               # buckets released before finish() (overlap actually happened)

    def _launch(self, top):
        import torch.distributed as dist
        while self.next + 1 < len(self.bounds) and self.bounds[self.next + 1] >= top:
            a, b = self.bounds[self.next + 1], self.bounds[self.next]
            self.works.append(dist.all_reduce(self.flat[a:b], op=dist.ReduceOp.SUM, async_op=True))
            self.next += 1

    def done(self, offsets):
        for off in offsets:
            self.pending.pop(off, None)
        before = len(self.works)
        self._launch(max(self.pending.values()) if self.pending else 0)
        self.early += len(self.works) - before

    def finish(self, wait=True):
        """launch what is left; wait=False returns the buckets' ranges in launch order instead (the caller waits per bucket)"""
        self._launch(0)
        if wait:
            for w in self.works:
                w.wait()
        return [(self.bounds[j + 1], self.bounds[j]) for j in range(len(self.works))]


def bucketed_allreduce(flat, n, bucket_elems):
    """Sum-all-reduce of the first n elements of a flat gradient buffer in fixed-size buckets (RCCL over xGMI on the GPU,
    gloo in the CPU tests).  The reference's nn.DataParallel reduce_add of the replicas' gradients (train.py:185) becomes
    one process per GPU + this call; unused parameters sit beyond n and are never communicated."""
    import torch.distributed as dist
    works = []
    for off in range(0, n, bucket_elems):
        works.append(dist.all_reduce(flat[off:min(n, off + bucket_elems)], op=dist.ReduceOp.SUM, async_op=True))
    for w in works:
        w.wait()
