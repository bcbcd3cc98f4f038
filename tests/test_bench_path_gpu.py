"""GPU parity of the exact configuration bench.py times, and the failure paths around it.

The headline step (bench.py main, config C1) is mdx_flow_warp_diff_batch_dev over 32 resident
1920x1080 gray pairs with the reference constants and pixel_step 10, called back to back without a
host sync and with call pipelining on.  That configuration engages machinery no smaller case does:
five pyramid levels, the LK level dataflow (batch a multiple of 8 and >= 16, 20736 points = a
multiple of 16, so level l-1's groups wait per pair on level l's retire counters; 4 pairs per XCD
range), level 0 on k_lk_iter<8, 112>, and alternating pyramid halves.  Every output of every pair
is compared with the oracle (reference optical_flow_calculator.cpp:71-127: calcOpticalFlowPyrLK,
classification, getPerspectiveTransform, warpPerspective, absdiff, threshold).

Also here: a dataflow hand-off that gives up is recovered within the call (the level is recomputed
in sequence: bit-exact, MDX_OK, counted by mdx_lk_fallbacks), and a pipelined call whose frames come
from a producer on another stream is correct once the producer's event is passed with
mdx_input_ready.
"""
import ctypes as C
from contextlib import ExitStack

import numpy as np
import pytest

from oracle_check import (NO_FALLBACKS, OutputSet, assert_batch_equals_oracle, lk_env, run_batch, uploaded,
                          without)

pytestmark = pytest.mark.gpu

W, H, B, PS = 1920, 1080, 32, 10


def _pairs(mdx, seeds, w, h):
    return {s: mdx.synth_pair(s, w, h, 1, 16) for s in seeds}


def _oracle_refs(oracle, pairs):
    return {s: oracle.calculate_optical_flow(a, b, nthreads=16, pixel_step=PS, min_vector_size=1.0)
            for s, (a, b, _) in pairs.items()}


def _stack(pairs, slot_seeds):
    g1 = np.stack([pairs[s][0] for s in slot_seeds])
    g2 = np.stack([pairs[s][1] for s in slot_seeds])
    return g1, g2


def test_benchmarked_path_1080p_x32_pipelined(mdx, oracle):
    """bench.py's timed step, twice back to back on different inputs (16 distinct pairs, 8 per call,
    each in 4 of the 32 slots), call pipelining on, one sync at the end: every pair's next_pts
    (float32 bits), status, H (float64 bits), mask and num_vectors -- and the Vec4d of the second
    call -- equal the oracle's."""
    seeds_a = [20141105 + i for i in range(8)]
    seeds_b = [20141205 + i for i in range(8)]
    pairs = _pairs(mdx, seeds_a + seeds_b, W, H)
    refs = _oracle_refs(oracle, pairs)
    slots_a = [seeds_a[i % 8] for i in range(B)]
    slots_b = [seeds_b[(3 * i + 1) % 8] for i in range(B)]      # another spread over the slots
    n = mdx.grid_count(W, H, PS)
    assert n % 16 == 0 and B % 8 == 0 and B >= 16               # the dataflow's conditions hold
    with mdx.Context(0, W, H, B, pixel_step=PS, min_vector_size=1.0, call_pipelining=1) as c, ExitStack() as stack:
        ins = [stack.enter_context(uploaded(c, *_stack(pairs, slots))) for slots in (slots_a, slots_b)]
        outs = [stack.enter_context(OutputSet(c, B, W, H, n, vectors=v)).prefill() for v in (False, True)]
        # a warm-up call into the second output set first, so that the two checked calls run with
        # the previous call still in flight (the bench's steady state)
        outs[1].call(*ins[1])
        outs[0].call(*ins[0])
        outs[1].call(*ins[1])
        c.sync()                                                # also the hand-off timeout check
        got = [o.read() for o in outs]
    assert_batch_equals_oracle(got[0], [refs[s] for s in slots_a], "call 0", fields=without("vectors"))
    assert_batch_equals_oracle(got[1], [refs[s] for s in slots_b], "call 1")


def _small_batch(mdx, w=320, h=240, batch=16, seed0=900):
    pairs = _pairs(mdx, [seed0 + i for i in range(batch)], w, h)
    slots = [seed0 + i for i in range(batch)]
    return pairs, slots


@pytest.mark.parametrize("spin", ["-1", "2"])
def test_dataflow_fallback_is_bit_exact(mdx, oracle, monkeypatch, spin):
    """The benchmarked configuration (1080p x 32, call pipelining on, two calls in flight) with the
    dataflow's waits forced to give up: MDX_LK_SPIN_MAX=-1 (read at mdx_create) makes every wait and
    gate give up at once, as when the coarser level's launch is never dispatched beside the finer
    one (a preempted, shared or kernel-serializing device); 2 polls makes some give up and others
    not.  Each abandoned level is recomputed in sequence within the same call (launch_lk_v2), so
    the sync reports MDX_OK and every output is bit-exact against the oracle; the fallback counts
    say what happened (for -1: every level below the coarsest recomputed, in every call)."""
    lk_env(monkeypatch, spin_max=spin)
    seeds_a = [20141105 + i for i in range(8)]
    seeds_b = [20141305 + i for i in range(8)]
    pairs = _pairs(mdx, seeds_a + seeds_b, W, H)
    refs = _oracle_refs(oracle, pairs)
    slots_a = [seeds_a[i % 8] for i in range(B)]
    slots_b = [seeds_b[(5 * i + 3) % 8] for i in range(B)]
    n = mdx.grid_count(W, H, PS)
    with mdx.Context(0, W, H, B, pixel_step=PS, min_vector_size=1.0, call_pipelining=1) as c, ExitStack() as stack:
        ins = [stack.enter_context(uploaded(c, *_stack(pairs, slots))) for slots in (slots_a, slots_b)]
        outs = [stack.enter_context(OutputSet(c, B, W, H, n)).prefill() for _ in range(2)]
        outs[0].call(*ins[0])
        outs[1].call(*ins[1])
        c.sync()                                                # MDX_OK: no exception
        fb = c.lk_fallbacks()
        got = [o.read() for o in outs]
    print("fallbacks:", fb)
    if spin == "-1":
        nlev = 5                                                # 1080p: levels 0..4
        assert fb["group_giveups"] > 0 and fb["gate_giveups"] == 2 * (nlev - 1)
        assert fb["levels_recomputed"] == 2 * (nlev - 1)
    for j, slots in enumerate((slots_a, slots_b)):
        assert_batch_equals_oracle(got[j], [refs[s] for s in slots], f"spin {spin} call {j}")


@pytest.mark.parametrize("spin,w,h,batch", [(None, 1920, 1080, 1), (None, 640, 480, 4), (None, 1920, 1080, 16),
                                             ("-1", 640, 480, 4)])
def test_small_batches_pipelined_back_to_back(mdx, oracle, monkeypatch, spin, w, h, batch):
    """Two pipelined calls back to back at small batches: 1 and 4 pairs, which the level dataflow
    does not take (it needs a multiple of 8 and at least 16 -- their levels run in sequence, so no
    hand-off can give up: the fallback counts stay 0), and 16, the smallest it does.  Also 4 pairs
    with MDX_LK_SPIN_MAX=-1, which must change nothing where no dataflow runs.  Bit-exact."""
    lk_env(monkeypatch, spin_max=spin)
    seeds = [31000 + i for i in range(min(batch, 4))]
    pairs = _pairs(mdx, seeds, w, h)
    refs = _oracle_refs(oracle, pairs)
    slots = [seeds[i % len(seeds)] for i in range(batch)]
    n = mdx.grid_count(w, h, PS)
    with mdx.Context(0, w, h, batch, pixel_step=PS, min_vector_size=1.0, call_pipelining=1) as c, ExitStack() as stack:
        d1, d2 = stack.enter_context(uploaded(c, *_stack(pairs, slots)))
        outs = [stack.enter_context(OutputSet(c, batch, w, h, n)).prefill() for _ in range(2)]
        for o in outs:
            o.call(d1, d2)
        c.sync()
        fb = c.lk_fallbacks()
        got = [o.read() for o in outs]
    if not spin and batch < 16:
        assert fb == NO_FALLBACKS
    for j in range(2):
        assert_batch_equals_oracle(got[j], [refs[sd] for sd in slots], f"{w}x{h} x{batch} spin {spin} call {j}")


def test_smaller_batch_behind_larger_pipelined(mdx, oracle):
    """A pipelined call of 8 pairs right behind one of 32 on the same context and frame size, one
    sync at the end.  The LK scratch is laid out by batch ([level][pair][point] A sums, the queue
    heads behind them), so the second call's aux-stream writes of one level fall into regions the
    first call's other levels still read -- with 8 pairs its level 1..3 A sums cover the first
    call's level-0 sums of pairs 8..31, and they wait only for the first call's levels 1..3: the
    layout change must let the first call finish first.  Every slot of both calls against the
    oracle, bit for bit."""
    w, h, b1, b2 = W, H, B, 8
    seeds = [32000 + i for i in range(8)]
    pairs = _pairs(mdx, seeds, w, h)
    refs = _oracle_refs(oracle, pairs)
    slots = [[seeds[i % 8] for i in range(b1)], [seeds[(3 * i + 5) % 8] for i in range(b2)]]
    n = mdx.grid_count(w, h, PS)
    with mdx.Context(0, w, h, b1, pixel_step=PS, min_vector_size=1.0, call_pipelining=1) as c, ExitStack() as stack:
        ins = [stack.enter_context(uploaded(c, *_stack(pairs, sl))) for sl in slots]
        outs = [stack.enter_context(OutputSet(c, b, w, h, n)) for b in (b1, b2)]
        # a warm-up call at the larger batch, so that the checked calls find every buffer allocated
        outs[0].call(*ins[0])
        c.sync()
        for o in outs:
            o.prefill()
        outs[0].call(*ins[0])
        outs[1].call(*ins[1])
        c.sync()
        got = [o.read() for o in outs]
    for j, sl in enumerate(slots):
        assert_batch_equals_oracle(got[j], [refs[s] for s in sl], f"call {j}")


def test_default_run_fallbacks_are_recovered(mdx, monkeypatch):
    """With the default wait bound the fallback counters are statistics, not errors: on an idle
    device they stay 0 (the bench reports them per run), while on a shared, preempted or
    profiler-serialized device a wait may give up -- then every give-up must have been followed by
    a recompute within the same call (mdx_sync would otherwise return MDX_EHIP)."""
    lk_env(monkeypatch)
    w, h, batch = 640, 480, 16
    pairs, slots = _small_batch(mdx, w, h, batch, seed0=990)
    fb = run_batch(mdx, *_stack(pairs, slots), create=dict(pixel_step=PS, min_vector_size=1.0, call_pipelining=1),
                   vectors=False, calls=4, back_to_back=True)["fallbacks"]
    print("lk_fallbacks", fb)
    if fb["group_giveups"] + fb["gate_giveups"] > 0:
        assert fb["levels_recomputed"] > 0, fb
    else:
        assert fb["levels_recomputed"] == 0, fb


def _hip():
    """The HIP runtime libmdx.so is linked against (already loaded: dlopen returns it)."""
    L = C.CDLL("libamdhip64.so")
    vp = C.c_void_p
    L.hipStreamCreate.argtypes = [C.POINTER(vp)]
    L.hipEventCreate.argtypes = [C.POINTER(vp)]
    L.hipHostMalloc.argtypes = [C.POINTER(vp), C.c_size_t, C.c_uint]
    L.hipMemcpyAsync.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
    L.hipEventRecord.argtypes = [vp, vp]
    L.hipStreamSynchronize.argtypes = [vp]
    L.hipStreamDestroy.argtypes = [vp]
    L.hipEventDestroy.argtypes = [vp]
    L.hipHostFree.argtypes = [vp]
    L.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
    L.hipFree.argtypes = [vp]
    return L


def test_input_ready_event_from_producer_stream(mdx, oracle):
    """Zero-copy producer on its own stream: a large copy queued first keeps that stream busy, the
    frames follow, an event is recorded behind them and handed over with mdx_input_ready.  The
    pipelined call (its front end on the context's second stream, not behind the context stream)
    waits for it: results bit-exact.  The device buffers hold zeros before the producer writes, so
    a front end that ran early would have read the wrong frames."""
    hip = _hip()
    w, h, batch = 640, 480, 16
    pairs, slots = _small_batch(mdx, w, h, batch, seed0=980)
    refs = _oracle_refs(oracle, pairs)
    n = mdx.grid_count(w, h, PS)
    g1, g2 = _stack(pairs, slots)
    vp = C.c_void_p
    st, ev, host, big_h, big_d = vp(), vp(), vp(), vp(), vp()
    BIG = 256 << 20
    assert hip.hipStreamCreate(C.byref(st)) == 0
    assert hip.hipEventCreate(C.byref(ev)) == 0
    assert hip.hipHostMalloc(C.byref(host), 2 * g1.nbytes, 0) == 0
    assert hip.hipHostMalloc(C.byref(big_h), BIG, 0) == 0
    try:
        hb = np.ctypeslib.as_array(C.cast(host, C.POINTER(C.c_uint8)), shape=(2 * g1.nbytes,))
        hb[:g1.nbytes] = g1.ravel()
        hb[g1.nbytes:] = g2.ravel()
        with mdx.Context(0, w, h, batch, pixel_step=PS, min_vector_size=1.0, call_pipelining=1) as c:
            assert hip.hipMalloc(C.byref(big_d), BIG) == 0
            z = np.zeros(g1.nbytes, np.uint8)
            with uploaded(c, z, z) as (d1, d2), OutputSet(c, batch, w, h, n) as o:
                o.prefill()
                assert hip.hipMemcpyAsync(big_d, big_h, BIG, 1, st) == 0          # keeps the producer busy
                assert hip.hipMemcpyAsync(vp(d1), host, g1.nbytes, 1, st) == 0
                assert hip.hipMemcpyAsync(vp(d2), vp(host.value + g1.nbytes), g2.nbytes, 1, st) == 0
                assert hip.hipEventRecord(ev, st) == 0
                c.input_ready(ev.value)
                o.call(d1, d2)
                c.sync()
                got = o.read()
                assert hip.hipStreamSynchronize(st) == 0
            hip.hipFree(big_d)
    finally:
        hip.hipHostFree(host)
        hip.hipHostFree(big_h)
        hip.hipEventDestroy(ev)
        hip.hipStreamDestroy(st)
    assert_batch_equals_oracle(got, [refs[s] for s in slots], "producer stream")
