"""The guarded-buffer helper of the output-contract tests, checked on the host: it must see one byte written in front
of a payload, one byte written behind it and one element left unwritten, and nothing when the payload is written fully and
only; and the case table of tests/test_output_contract_gpu.py must exercise what those tests are about -- episode ends
in the middle of a batch, ends by success, lifelong respawns -- which is decided here from the CPU oracle alone, so that
no GPU case passes vacuously."""

from __future__ import annotations

import numpy as np
import pytest

import guard_util as gu

BACKENDS = ["cpu", "numpy"]
DTYPES = [np.float32, np.float64, np.uint8, np.int8, np.int16, np.int32, np.int64]


def _write_all(buf, value=1):
    v = buf.payload_view()
    v[...] = value


@pytest.mark.parametrize("device", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fully_and_only_written_payload_reports_nothing(device, dtype):
    buf = gu.GuardedBuffer((5, 3), dtype, device, name="out")
    assert buf.address % 256 == gu.PAYLOAD_PHASE and buf.guard_bytes >= gu.MIN_GUARD
    assert buf.guards_intact() and buf.unwritten().all() and buf.unwritten().shape == (5, 3)
    _write_all(buf)
    assert buf.guards_intact() and not buf.unwritten().any()
    assert np.array_equal(buf.check(True), np.ones((5, 3), dtype))
    buf.poison()
    assert buf.unwritten().all()
    buf.check(False)


def test_poison_is_no_value_an_output_can_hold():
    for dtype in DTYPES:
        v = gu.GuardedBuffer((1,), dtype, "numpy").array()[0]
        assert v < 0 or (np.dtype(dtype) == np.uint8 and v == 165), (dtype, v)
        if np.dtype(dtype).kind == "f":
            assert -1e-15 < v < 0  # no reward, observation or info value


@pytest.mark.parametrize("device", BACKENDS)
def test_one_byte_in_front_of_the_payload_is_reported(device):
    buf = gu.GuardedBuffer((4, 2), np.float32, device, name="rewards")
    _write_all(buf)
    buf.arena[buf.offset - 1] = 0
    assert not buf.guards_intact()
    with pytest.raises(AssertionError, match=r"BEFORE rewards, nearest 1 byte"):
        buf.check(True)
    buf.poison()
    buf.arena[0] = 7  # the far end of the guard counts as well
    with pytest.raises(AssertionError, match="BEFORE rewards"):
        buf.check(False)


@pytest.mark.parametrize("device", BACKENDS)
def test_one_byte_behind_the_payload_is_reported(device):
    buf = gu.GuardedBuffer((6,), np.uint8, device, name="truncated")
    _write_all(buf, 0)
    buf.arena[buf.offset + buf.nbytes] = 1
    assert not buf.guards_intact()
    with pytest.raises(AssertionError, match=r"AFTER truncated, first 0 byte\(s\) past its end = flat element 6 of 6"):
        buf.check(True)
    buf.poison()
    buf.arena[len(buf.arena) - 1] = 1
    with pytest.raises(AssertionError, match="AFTER truncated"):
        buf.check(False)


@pytest.mark.parametrize("device", BACKENDS)
def test_one_unwritten_element_is_reported_with_its_index(device):
    buf = gu.GuardedBuffer((3, 14), np.float32, device, name="info_all")
    _write_all(buf, 0.0)
    v = buf.payload_view()
    raw = buf.arena[buf.offset + (2 * 14 + 13) * 4: buf.offset + (2 * 14 + 13) * 4 + 4]
    raw[...] = gu.POISON
    un = buf.unwritten()
    assert un.sum() == 1 and un[2, 13]
    with pytest.raises(AssertionError, match=r"info_all.*must write are still poison, first index \[2, 13\]"):
        buf.check(True)
    # three of an element's four bytes left: the element counts as written
    raw[0:1] = 0
    assert not buf.unwritten().any()
    del v


@pytest.mark.parametrize("device", BACKENDS)
def test_row_masks_and_stray_writes(device):
    buf = gu.GuardedBuffer((4, 2, 3), np.float32, device, name="final_obs")
    v = buf.payload_view()
    v[1] = 0.5
    v[3] = 0.25
    buf.check(np.array([False, True, False, True]))
    with pytest.raises(AssertionError, match=r"final_obs.*must leave alone were written, first index \[3, 0, 0\]"):
        buf.check(np.array([False, True, False, False]))
    with pytest.raises(AssertionError, match=r"still poison, first index \[0, 0, 0\]"):
        buf.check(np.array([True, True, False, True]))


def test_two_fill_rule_sees_an_element_that_keeps_the_old_content():
    buf = gu.GuardedBuffer((2, 4, 4, 3), np.uint8, "numpy", name="frames")

    def full():
        buf.payload_view()[...] = 165  # the poison byte itself is a legitimate pixel value

    assert (gu.two_fill(buf, full) == 165).all()

    def leaves_one():
        v = buf.payload_view()
        keep = v[1, 2, 3, 0]
        v[...] = 165
        v[1, 2, 3, 0] = keep

    with pytest.raises(AssertionError, match=r"frames.*first index \[1, 2, 3, 0\]"):
        gu.two_fill(buf, leaves_one)


def test_guard_holds_a_whole_slab():
    assert gu.guard_bytes_for(10) == 4096
    assert gu.guard_bytes_for(23 * 8 * 33 * 4) == (23 * 8 * 33 * 4 + 255) // 256 * 256
    bufs = gu.guarded_outputs(gu.ma_output_specs(23, 8, 33), "cpu", lead=(7,))
    assert bufs["obs"].shape == (7, 23, 8, 33) and bufs["obs"].guard_bytes >= 23 * 8 * 33 * 4
    assert bufs["terminated"].guard_bytes == 4096


# ---- the case table, from the oracle alone -------------------------------------------------------------------------------
def test_case_table_names_every_path_once():
    ids = [c["id"] for c in gu.CASES]
    assert len(set(ids)) == len(ids)
    for c in gu.CASES:
        assert c["H"] <= 12 and c["W"] <= 12 and c["H"] != c["W"] or (c["H"], c["W"]) in ((5, 64), (12, 12)), c["id"]
        assert 5 <= c["cfg"]["steps_per_episode"] <= 9, c["id"]
        G = 64 // c["lanes"]
        if not c.get("batches"):
            assert gu.case_batches(c) == ((1, 3) if G == 1 else (1, G + 1, 3 * G - 1))
    small = [c for c in gu.MA_CASES if c["lanes"] <= 16]
    assert any(c["cfg"].get("deterministic") for c in small) and any(c["cfg"].get("lifelong_mapf") for c in small)


@pytest.fixture(scope="module")
def coverage():
    return {(c["id"], B): gu.coverage_of(c, B) for c in gu.CASES for B in gu.case_batches(c)}


@pytest.mark.parametrize("cid,B", gu.case_params())
def test_case_meets_its_coverage_conditions(coverage, cid, B):
    cov = coverage[(cid, B)]
    assert cov["episode_ends"] >= 2 * B, cov
    if B > 1:  # (a batch of one env has no step in which some envs finish and others do not)
        assert cov["mixed_steps"] >= 1, cov
    if gu.CASE_BY_ID[cid]["cfg"].get("lifelong_mapf"):
        assert cov["respawns"] >= 1, cov


def test_some_finite_episode_ends_in_success(coverage):
    for kind in ("ma", "cte"):
        n = sum(v["successes"] for (cid, _), v in coverage.items()
                if gu.CASE_BY_ID[cid]["kind"] == kind and not gu.CASE_BY_ID[cid]["cfg"].get("lifelong_mapf"))
        assert n >= 1, kind
