"""tests/oracle_check.py on the CPU: the comparisons are not vacuous (one changed bit of any field
fails, with the label in the message), and the output set and the runner, against a fake context over
numpy-backed "device" memory, free what they allocate and prefill before the entry runs."""
import types

import numpy as np
import pytest

import oracle_check as oc

N, MW, MH = 6, 8, 6


def _ref():
    rng = np.random.default_rng(5)
    return dict(num_vectors=4, status=np.array([1, 1, 0, 1, 1, 0], np.uint8),
                next_pts=rng.uniform(1, 50, (N, 2)).astype(np.float32),
                vectors=np.zeros((N, 4)) + [3.0, 4.0, 0.0, 1.5], H=np.eye(3) + rng.uniform(-0.1, 0.1, (3, 3)),
                mask=(rng.integers(0, 2, (MH, MW)) * 255).astype(np.uint8), why=np.arange(N, dtype=np.uint16))


def _copy(ref):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ref.items() if k != "why"}


CHANGES = ["next_pts", "vectors", "H", "status", "mask", "num_vectors+", "num_vectors-"]


def _changed(change):
    """A copy of _ref() with one smallest change in the named field."""
    g = _copy(_ref())
    if change == "next_pts":
        g["next_pts"].view(np.uint32)[2, 1] ^= 1                  # the lowest mantissa bit of one float
    elif change == "vectors":
        assert g["vectors"][3, 2] == 0.0
        g["vectors"][3, 2] = -0.0
    elif change == "H":
        g["H"][1, 2] = np.nextafter(g["H"][1, 2], 2.0)            # one ulp
    elif change == "status":
        g["status"][4] ^= 1
    elif change == "mask":
        g["mask"][5, 7] ^= 255
    else:
        g["num_vectors"] += 1 if change == "num_vectors+" else -1
    return g


def test_equal_pair_passes():
    ref = _ref()
    oc.assert_pair_equals_oracle(_copy(ref), ref, "same")
    oc.assert_pair_equals_oracle(types.SimpleNamespace(**_copy(ref)), ref, "same, as a result object")


@pytest.mark.parametrize("change", CHANGES)
def test_one_changed_bit_fails(change):
    ref, got = _ref(), _changed(change)
    with pytest.raises(AssertionError, match="case-label"):
        oc.assert_pair_equals_oracle(got, ref, "case-label")
    if change == "next_pts":
        with pytest.raises(AssertionError, match=r"1 LK points differ, first \[2\].*why \[2\]"):
            oc.assert_pair_equals_oracle(got, ref, "case-label")


@pytest.mark.parametrize("change", CHANGES)
def test_fields_leave_out_exactly_one(change):
    """Leaving a field out lets its change pass, and no other field's."""
    field = change.rstrip("+-")
    ref, got = _ref(), _changed(change)
    oc.assert_pair_equals_oracle(got, ref, "left out", fields=oc.without(field))
    for other in oc.without(field):
        with pytest.raises(AssertionError, match="kept"):
            oc.assert_pair_equals_oracle(got, ref, "kept", fields=oc.without(other))


def test_a_missing_field_is_not_skipped():
    ref, got = _ref(), _copy(_ref())
    got["mask"] = None                       # a host call with want_mask=False
    with pytest.raises(ValueError, match="mask"):
        oc.assert_pair_equals_oracle(got, ref, "no mask")
    oc.assert_pair_equals_oracle(got, ref, "no mask", fields=oc.without("mask"))
    del got["vectors"]                       # a batch read-back without the vectors buffer
    with pytest.raises(ValueError, match="vectors"):
        oc.assert_pair_equals_oracle(got, ref, "no vectors", fields=["vectors"])
    with pytest.raises(ValueError, match="unknown"):
        oc.assert_pair_equals_oracle(got, ref, "typo", fields=["statuz"])


def _traj():
    rng = np.random.default_rng(9)
    ref = dict(num_vectors=3, traj=rng.uniform(1, 50, (N, 4, 2)).astype(np.float32),
               traj_len=np.array([4, 1, 3, 4, 2, 4], np.int32), start_pts=rng.uniform(1, 50, (N, 2)).astype(np.float32),
               vectors=np.zeros((N, 4)) + [3.0, 4.0, 0.0, 1.5])
    return ref, types.SimpleNamespace(**{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ref.items()})


def test_trajectory_form():
    ref, res = _traj()
    oc.assert_traj_equals_oracle(res, ref, "same")
    res.traj.view(np.uint32)[2, 3, 0] ^= 1           # index traj_len[2]: not part of the result
    oc.assert_traj_equals_oracle(res, ref, "past the end")
    res.traj.view(np.uint32)[2, 2, 0] ^= 1           # index traj_len[2] - 1
    with pytest.raises(AssertionError, match="traj-label: point 2"):
        oc.assert_traj_equals_oracle(res, ref, "traj-label")
    for change in (lambda r: r.traj_len.__setitem__(1, 2), lambda r: r.start_pts.view(np.uint32).__setitem__((0, 0), 7),
                   lambda r: r.vectors.__setitem__((5, 2), -0.0), lambda r: setattr(r, "num_vectors", 2)):
        ref, res = _traj()
        change(res)
        with pytest.raises(AssertionError, match="traj-label"):
            oc.assert_traj_equals_oracle(res, ref, "traj-label")


class FakeContext:
    """dev_alloc / dev_free / h2d / d2h over numpy arrays, and a batch entry that records what its
    outputs held when it was called, then writes byte 0x10 + call index over each of them."""

    def __init__(self, fail_on_call=None, fail_on_alloc=None):
        self.mem, self.freed, self.next_ptr, self.fail_on_alloc = {}, [], 0x1000, fail_on_alloc
        self.calls, self.h2d_log, self.fail_on_call = [], [], fail_on_call
        self.params = types.SimpleNamespace(pixel_step=10)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def dev_alloc(self, nbytes):
        if len(self.mem) == self.fail_on_alloc:
            raise MemoryError("out of device memory")
        p, self.next_ptr = self.next_ptr, self.next_ptr + 0x100000
        self.mem[p] = np.zeros(nbytes, np.uint8)
        return p

    def dev_free(self, p):
        del self.mem[p]
        self.freed.append(p)

    def h2d(self, dst, src):
        self.h2d_log.append((dst, len(self.calls)))
        self.mem[dst][:] = np.ascontiguousarray(src).view(np.uint8).ravel()

    def d2h(self, dst, src):
        dst.view(np.uint8).ravel()[:] = self.mem[src]

    def sync(self):
        pass

    def lk_fallbacks(self):
        return dict(oc.NO_FALLBACKS)

    def flow_warp_diff_batch_dev(self, batch, d_img1, d_img2, w, h, stride, frame_stride, fmt, **outs):
        assert set(outs) == {"d_next_pts", "d_status", "d_vectors", "d_mask", "d_H", "d_num_vectors"}
        seen = {k: bool((self.mem[p] == 0xAA).all()) for k, p in outs.items() if p}
        self.calls.append(dict(args=(batch, w, h, stride, frame_stride, fmt), outs=outs, all_aa=seen))
        if self.fail_on_call == len(self.calls):
            raise RuntimeError("entry failed")
        for p in outs.values():
            if p:
                self.mem[p][:] = 0x10 + len(self.calls) - 1


def _fake_mdx(fake):
    return types.SimpleNamespace(Context=lambda dev, w, h, batch, **kw: fake,
                                 grid_count=lambda w, h, ps: ((w + ps - 1) // ps) * ((h + ps - 1) // ps))


FRAMES = np.zeros((3, 20, 30), np.uint8)         # batch 3, 30 x 20, 6 points at pixel_step 10


@pytest.mark.parametrize("fail_on_call", [1, 2])
def test_everything_is_freed_when_the_entry_raises(fail_on_call):
    fake = FakeContext(fail_on_call)
    with pytest.raises(RuntimeError, match="entry failed"):
        oc.run_batch(_fake_mdx(fake), FRAMES, FRAMES, calls=2)
    assert len(fake.calls) == fail_on_call and len(fake.freed) == 8 and not fake.mem


def test_outputs_are_prefilled_before_each_call():
    fake = FakeContext()
    got = oc.run_batch(_fake_mdx(fake), FRAMES, FRAMES, calls=3)
    assert len(fake.calls) == 3 and not fake.mem
    for call in fake.calls:
        assert len(call["all_aa"]) == 6 and all(call["all_aa"].values()), call["all_aa"]
        assert call["args"] == (3, 30, 20, 30, 600, 0)
    assert all((got[k].view(np.uint8) == 0x12).all() for k in oc.PAIR_FIELDS)       # the last call's
    assert got["fallbacks"] == oc.NO_FALLBACKS


def test_back_to_back_prefills_once_and_copies_nothing_between_calls():
    fake = FakeContext()
    oc.run_batch(_fake_mdx(fake), FRAMES, FRAMES, calls=2, back_to_back=True)
    assert all(fake.calls[0]["all_aa"].values()) and not any(fake.calls[1]["all_aa"].values())
    assert all(ncalls == 0 for _, ncalls in fake.h2d_log)


def test_without_vectors_there_is_no_such_buffer():
    fake = FakeContext()
    got = oc.run_batch(_fake_mdx(fake), FRAMES, FRAMES, vectors=False)
    assert fake.calls[0]["outs"]["d_vectors"] == 0 and len(fake.calls[0]["all_aa"]) == 5
    assert "vectors" not in got and len(fake.freed) == 7 and not fake.mem
    assert "vectors" not in oc.OutputSet.slot(got, 0)
    with pytest.raises(AssertionError, match="2 refs for 3 slots"):
        oc.assert_batch_equals_oracle(got, [_ref()] * 2, "short", fields=oc.without("vectors"))


def test_read_gives_the_shapes_and_dtypes_the_tests_use():
    fake = FakeContext()
    with oc.OutputSet(fake, 3, 30, 20, 6) as out:
        out.prefill()
        got = out.read()
    assert not fake.mem
    want = dict(next_pts=((3, 6, 2), np.float32), status=((3, 6), np.uint8), vectors=((3, 6, 4), np.float64),
                mask=((3, 20, 30), np.uint8), H=((3, 3, 3), np.float64), num_vectors=((3,), np.int32))
    assert {k: (v.shape, v.dtype) for k, v in got.items()} == {k: (s, np.dtype(d)) for k, (s, d) in want.items()}
    assert all((v.view(np.uint8) == 0xAA).all() for v in got.values())
    one = oc.OutputSet.slot(got, 2)
    assert one["H"].shape == (3, 3) and one["mask"].shape == (20, 30) and one["num_vectors"].shape == ()


def test_a_failed_allocation_frees_the_earlier_ones():
    fake = FakeContext(fail_on_alloc=3)
    with pytest.raises(MemoryError):
        oc.OutputSet(fake, 3, 30, 20, 6)
    assert not fake.mem and len(fake.freed) == 3
