"""The GPU parity tests' oracle check, written once: the device output set of the zero-copy batch entry
(mdx_flow_warp_diff_batch_dev), the runner of its common case, and the comparisons of a pair's and a
trajectory's outputs with the oracle's (bit patterns, not values).

A new parity test is three lines:

    got = run_batch(mdx, g1, g2, create=dict(pixel_step=10, min_vector_size=1.0))
    for i in range(len(g1)):
        assert_pair_equals_oracle(OutputSet.slot(got, i), refs[i], f"pair {i}")

Every output buffer is filled with 0xAA before the entry runs and compared whole, so an element no
kernel writes fails instead of passing on whatever the allocation held.
"""
import contextlib
import ctypes as C

import numpy as np

PAIR_FIELDS = ("num_vectors", "status", "next_pts", "vectors", "H", "mask")
NO_FALLBACKS = {"group_giveups": 0, "gate_giveups": 0, "levels_recomputed": 0}


def without(*names):
    """PAIR_FIELDS less the named ones: the `fields` of a caller that did not produce them."""
    return tuple(f for f in PAIR_FIELDS if f not in names)


def lk_env(monkeypatch, fma="1", debug=False, spin_max=None):
    """The LK knobs read at mdx_create, each put into the stated state: MDX_LK_FMA ("0": the exact
    body everywhere; anything else: unset, the default choice), MDX_LK_DEBUG (the body counters) and
    MDX_LK_SPIN_MAX (None: unset, the default wait bound)."""
    for name, value in (("MDX_LK_FMA", "0" if fma == "0" else None), ("MDX_LK_DEBUG", "1" if debug else None),
                        ("MDX_LK_SPIN_MAX", spin_max)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


@contextlib.contextmanager
def uploaded(ctx, *arrays):
    """Device copies of the arrays -> their device pointers; freed on exit, also when the body raises."""
    ptrs = []
    try:
        for a in arrays:
            ptrs.append(ctx.dev_alloc(a.nbytes))
            ctx.h2d(ptrs[-1], a)
        yield ptrs
    finally:
        for p in ptrs:
            ctx.dev_free(p)


class OutputSet:
    """The device outputs of one batch-entry call: `batch` pairs of a w x h frame with n grid points.
    Without `vectors` there is no such buffer and the entry gets a null pointer for it.  A context
    manager: every allocation is released on exit (or by free())."""

    def __init__(self, ctx, batch, w, h, n, vectors=True):
        self.ctx, self.batch, self.w, self.h = ctx, batch, w, h
        self.layout = dict(next_pts=((batch, n, 2), np.float32), status=((batch, n), np.uint8),
                           vectors=((batch, n, 4), np.float64), mask=((batch, h, w), np.uint8),
                           H=((batch, 3, 3), np.float64), num_vectors=((batch,), np.int32))
        if not vectors:
            del self.layout["vectors"]
        self.dev = {}
        try:
            for k in self.layout:
                self.dev[k] = ctx.dev_alloc(self._nbytes(k))
        except BaseException:
            self.free()
            raise

    def _nbytes(self, k):
        shape, dtype = self.layout[k]
        return int(np.prod(shape)) * np.dtype(dtype).itemsize

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def free(self):
        while self.dev:
            self.ctx.dev_free(self.dev.popitem()[1])

    def prefill(self):
        """0xAA over every byte of every buffer (h2d returns after the copy, behind all earlier work
        of the context's stream) -> self."""
        for k, p in self.dev.items():
            self.ctx.h2d(p, np.full(self._nbytes(k), 0xAA, np.uint8))
        return self

    def call(self, d_img1, d_img2, stride=None, frame_stride=None, fmt=0):
        """The batch entry on this set; packed gray frames unless told otherwise."""
        stride = self.w if stride is None else stride
        frame_stride = stride * self.h if frame_stride is None else frame_stride
        return self.ctx.flow_warp_diff_batch_dev(
            self.batch, d_img1, d_img2, self.w, self.h, stride, frame_stride, fmt, d_next_pts=self.dev["next_pts"],
            d_status=self.dev["status"], d_vectors=self.dev.get("vectors", 0), d_mask=self.dev["mask"],
            d_H=self.dev["H"], d_num_vectors=self.dev["num_vectors"])

    def read(self):
        """Every buffer, whole: next_pts (batch, n, 2) float32, status (batch, n) uint8, vectors
        (batch, n, 4) float64, mask (batch, h, w) uint8, H (batch, 3, 3) float64, num_vectors (batch,)
        int32."""
        got = {k: np.empty(shape, dtype) for k, (shape, dtype) in self.layout.items()}
        for k, a in got.items():
            self.ctx.d2h(a, self.dev[k])
        return got

    @staticmethod
    def slot(got, i):
        """Pair i's view of a read-back."""
        return {k: got[k][i] for k in PAIR_FIELDS if k in got}


def run_batch(mdx, g1, g2, create=None, set_params=None, *, vectors=True, calls=1, back_to_back=False,
              body_counts=False):
    """The batch entry over the stacked packed gray frames g1, g2 (batch, h, w) on a context of its own,
    made `calls` times into one output set -> its read-back, plus "fallbacks" (lk_fallbacks() after the
    sync) and, with body_counts, "body_counts" (mdx_debug_copy item 6: [level][exact, fused]; needs
    MDX_LK_DEBUG).  `create` holds the keyword parameters given to Context(...), `set_params` those
    given to set_params() after it.

    The outputs are prefilled before each call.  The prefill is a copy on the context's stream, which
    the host waits for, so the calls then run one after another.  back_to_back keeps them enqueued
    without a host sync in between (what call pipelining overlaps): the outputs are prefilled before
    the first call only, and an element is caught if no call writes it."""
    batch, h, w = g1.shape
    with mdx.Context(0, w, h, batch, **(create or {})) as c:
        if set_params:
            c.set_params(**set_params)
        n = mdx.grid_count(w, h, c.params.pixel_step)
        with uploaded(c, g1, g2) as (d1, d2), OutputSet(c, batch, w, h, n, vectors) as out:
            for k in range(calls):
                if k == 0 or not back_to_back:
                    out.prefill()
                out.call(d1, d2)
            c.sync()
            got = out.read()
            got["fallbacks"] = c.lk_fallbacks()
            if body_counts:
                cnt = np.zeros((8, 2), np.uint32)
                rc = mdx.lib().mdx_debug_copy(c._h, 6, cnt.ctypes.data_as(C.c_void_p), cnt.nbytes)
                assert rc == 0
                got["body_counts"] = cnt
    return got


def _assert_same_bits(a, b, utype, what):
    """a and b (floats of one shape) hold the same bit patterns: -0.0 is not 0.0, a NaN equals only
    the same NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.dtype}{a.shape} vs {b.dtype}{b.shape}"
    bad = np.argwhere(a.view(utype) != b.view(utype))
    if bad.size:
        first = [tuple(map(int, i)) for i in bad[:3]]
        raise AssertionError(f"{what}: {len(bad)} entries differ in bits, first at {first}: "
                             f"{[a[i] for i in first]} vs {[b[i] for i in first]}")


def assert_pair_equals_oracle(got, ref, label, fields=PAIR_FIELDS):
    """One pair's outputs -- a FlowResult (host entries) or a slot of a batch read-back -- equal the
    oracle's `ref`, bit for bit, in every field of `fields`.  A field the caller did not produce (no
    mask from want_mask=False, no vectors buffer) has to be left out of `fields` by name."""
    if set(fields) - set(PAIR_FIELDS):
        raise ValueError(f"unknown fields {sorted(set(fields) - set(PAIR_FIELDS))}")
    if not isinstance(got, dict):
        got = {f: getattr(got, f) for f in PAIR_FIELDS}
    for f in fields:
        if got.get(f) is None:
            raise ValueError(f"{label}: no {f} was produced; leave it out of fields by name")
    if "num_vectors" in fields:
        assert int(got["num_vectors"]) == int(ref["num_vectors"]), \
            f"{label}: num_vectors {int(got['num_vectors'])} vs {int(ref['num_vectors'])}"
    if "status" in fields:
        np.testing.assert_array_equal(got["status"], ref["status"], err_msg=f"{label}: status")
    if "next_pts" in fields:
        assert got["next_pts"].shape == ref["next_pts"].shape, f"{label}: next_pts {got['next_pts'].shape}"
        bad = np.nonzero((got["next_pts"].view(np.uint32) != ref["next_pts"].view(np.uint32)).any(axis=1))[0]
        if bad.size:
            why = f" why {ref['why'][bad[:3]]}" if "why" in ref else ""
            raise AssertionError(f"{label}: {bad.size} LK points differ, first {bad[:5]}: "
                                 f"{got['next_pts'][bad[:3]]} vs {ref['next_pts'][bad[:3]]}{why}")
    if "vectors" in fields:
        _assert_same_bits(got["vectors"], ref["vectors"], np.uint64, f"{label}: vectors")
    if "H" in fields:
        _assert_same_bits(got["H"].reshape(3, 3), ref["H"].reshape(3, 3), np.uint64, f"{label}: H")
    if "mask" in fields:
        assert got["mask"].shape == ref["mask"].shape, f"{label}: mask {got['mask'].shape}"
        nbad = int((got["mask"] != ref["mask"]).sum())
        assert nbad == 0, f"{label}: {nbad} mask pixels differ"


def assert_batch_equals_oracle(got, refs, label, fields=PAIR_FIELDS):
    """Slot i of a batch read-back equals refs[i], for every slot."""
    assert len(refs) == len(got["num_vectors"]), f"{label}: {len(refs)} refs for {len(got['num_vectors'])} slots"
    for i, ref in enumerate(refs):
        assert_pair_equals_oracle(OutputSet.slot(got, i), ref, f"{label} slot {i}", fields)


def assert_traj_equals_oracle(res, ref, label):
    """A TrajectoryResult equals the oracle's: the lengths, each trajectory up to its length (entries
    past it are not part of the result), the last pass's start points and Vec4d, num_vectors."""
    np.testing.assert_array_equal(res.traj_len, ref["traj_len"], err_msg=f"{label}: traj_len")
    for i in range(len(res.traj_len)):
        k = int(ref["traj_len"][i])
        a, b = res.traj[i, :k].view(np.uint32), ref["traj"][i, :k].view(np.uint32)
        assert np.array_equal(a, b), f"{label}: point {i}: {res.traj[i, :k]} vs {ref['traj'][i, :k]}"
    _assert_same_bits(res.start_pts, ref["start_pts"], np.uint32, f"{label}: start_pts")
    _assert_same_bits(res.vectors, ref["vectors"], np.uint64, f"{label}: vectors")
    assert res.num_vectors == ref["num_vectors"], f"{label}: num_vectors {res.num_vectors} vs {ref['num_vectors']}"
