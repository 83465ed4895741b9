"""Shared drivers of the -m gpu tests: a target-sharded align() with a REAL second rank on
a one-GPU box (two contexts, two host threads)."""
import ctypes
import threading

import numpy as np

from loop_ref_cases import snap as _snap


def align_two_ranks(pkg, mode, xf, ff, xm, fm, exchange="mailbox", timeout=300, world=2, cuts=None, mcuts=None, params=None,
                    trace_cap=0, barrier_timeout=None, options=None, chain=None):
    """Runs `world` contexts on GPU 0, context r holding rows shard_range(n, r, world) of the
    fixed cloud (and of the moving cloud for the acvo Ayy rows), each from its own host thread.

    cuts / mcuts: cut lists of the fixed / the moving rows instead (tests/shard_cases.py: rank r holds [cuts[r], cuts[r + 1]),
    world = len(cuts) - 1); params: the contexts' parameters (mode is then theirs); trace_cap: records kept per rank;
    barrier_timeout: seconds every barrier.wait of a rank may take (default: `timeout`) -- a rank that runs one exchange more
    than its peers, or does not come at all, ends as threading.BrokenBarrierError in its peers and a failure here, not
    as a wait; options: {key: value} for cvo_hip_set_option on every rank; chain: a list of Params -- after the registration
    every rank runs one more per entry on the SAME contexts, streams and exchange (cvo_hip_set_params, a fresh state), all
    ranks entering each together.

    exchange = "mailbox": cvo_hip_mailbox_create / _connect -- the partial sums travel through
               device-memory mailboxes inside the launch chain (the peer-store all-reduce that
               runs over xGMI between GPUs; here every mailbox lives on the one device);
    exchange = "hook":    cvo_hip_set_allreduce with a host-memory sum in rank order.

    Returns {rank: (iterations, bytes(state), transform 4x4, all-reduce calls, trace, state before, state after (both as
    loop_ref_cases.snap has them), list_stats(), [the same eight of every registration of `chain`])}."""
    capi = pkg.capi
    import torch
    n, m = len(xf), len(xm)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    if cuts is not None:
        world = len(cuts) - 1
        mcuts = mcuts if mcuts is not None else tuple(m * r // world for r in range(world + 1))
        assert len(mcuts) == len(cuts)
    barrier = threading.Barrier(world, timeout=barrier_timeout if barrier_timeout is not None else timeout)
    box = [None] * world
    boxes = [None] * world
    out = {}
    calls = [0] * world
    errors = []

    def rank(r):
        try:
            # (a stream of the library's own, created here and now: the ranks' streams are made back to back and land on hardware
            # queues of their own.  Streams from torch's pool -- 32 of them, handed out in turn to whoever asks in the process --
            # put two ranks on ONE hardware queue on some boxes: a rank that spins for its peer inside a kernel then keeps that
            # peer's kernels from ever starting, and both time out.  Ranks that share a GPU exist in tests only.)
            import os
            s = torch.cuda.Stream() if os.environ.get("RANK_TORCH_STREAM") else None
            c = capi.Context(params=params, mode=mode, device=0, stream=s.cuda_stream if s is not None else None)
            for key, value in (options or {}).items():
                c.set_option(key, value)
            c.set_fixed(xf, ff)
            c.set_moving(xm, fm)
            if cuts is not None:
                lo, hi, slo, shi = cuts[r], cuts[r + 1], mcuts[r], mcuts[r + 1]
            else:
                lo, hi = capi.shard_range(n, r, world)
                slo, shi = capi.shard_range(m, r, world)
            c.set_shard(lo, hi, slo, shi)
            if exchange == "mailbox":
                boxes[r] = c.mailbox_create(r, world)[1]
                barrier.wait()
                c.mailbox_connect(ptrs=list(boxes))
                barrier.wait()
            else:
                def hook(ptr, count, stream):
                    calls[r] += 1
                    hip.hipStreamSynchronize(stream)
                    mine = np.zeros(count, np.float64)
                    assert hip.hipMemcpy(mine.ctypes.data, ptr, count * 8, 2) == 0      # device -> host
                    box[r] = mine
                    try:
                        barrier.wait()
                        total = box[0].copy()
                        for q in range(1, world):
                            total = total + box[q]                                      # rank order
                        barrier.wait()
                    except threading.BrokenBarrierError:
                        # (raised on: the binding turns it into a failed all-reduce, and align() ends with CVO_HIP_ERR_COMM)
                        errors.append((r, "a peer did not come to exchange %d (%d values)" % (calls[r], count)))
                        raise
                    assert hip.hipMemcpy(ptr, total.ctypes.data, count * 8, 1) == 0     # host -> device
                c.set_allreduce(hook)
            def register():
                st = capi.init_state(c.params)
                s0 = _snap(st)
                before = calls[r]
                it, tr = c.align(st, trace_cap=trace_cap)
                return (it, bytes(st), np.array(st.transform, np.float32).reshape(4, 4), calls[r] - before, tr, s0, _snap(st), c.list_stats())
            first = register()
            more = []
            for p in chain or []:
                barrier.wait()
                c.set_params(p)
                more.append(register())
            out[r] = first + (more,)
            barrier.wait()   # nobody frees a mailbox a peer may still be writing to
            c.close()
        except Exception as e:   # pragma: no cover
            errors.append((r, repr(e)))
            barrier.abort()

    ts = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=timeout)
    assert not errors, errors
    assert sorted(out) == list(range(world)), "a rank did not finish"
    return out


def align_two_ranks_mailbox(pkg, mode, xf, ff, xm, fm, **kw):
    return align_two_ranks(pkg, mode, xf, ff, xm, fm, exchange="mailbox", **kw)
