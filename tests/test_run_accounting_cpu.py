# coding=utf-8
"""
The stopping rule's acceptance accounting of ``Run`` (lib/run.py:344-359) and its count of valid
chain slots, without a device.  The rule: iteration 1 of a segment counts every spaxel of every
chain as accepted; the rate at iteration i is accepted / (spaxels * chains * i), both over the
WHOLE chain -- a resumed segment adds to the totals of its state, which already hold its own
iteration 1.  Every expected number below is worked by hand from that rule.
"""
import numpy as np
import pytest

import deconv3d_amd as d3d
from deconv3d_amd.run import _Acceptance


def fresh_segment():
    acc = _Acceptance(5, 2)
    for per_chain in ([3, 1], [2, 2], [0, 4]):
        acc.add(per_chain)
    return acc


def test_a_fresh_segment_counts_its_first_iteration_as_accepted():
    acc = _Acceptance(5, 2)
    assert acc.running_rate(1) == 1.0                   # 10 / (10 * 1)
    acc.add([3, 1])
    assert acc.running_rate(2) == 14 / 20.
    acc.add([2, 2])
    assert acc.running_rate(3) == 18 / 30.
    acc.add([0, 4])
    pooled, per_chain = acc.final_rates(4)
    assert pooled == 22 / 40. and per_chain == [10 / 20., 12 / 20.]
    record = acc.state_record(4)
    assert sorted(record) == ["accepted_count", "per_chain_accepted", "total_accepted", "total_iterations"]
    assert (record["accepted_count"], record["total_accepted"], record["total_iterations"]) == (22, 22, 4)
    assert record["per_chain_accepted"].dtype == np.int64 and list(record["per_chain_accepted"]) == [10, 12]


def test_one_chain_has_one_rate_and_records_no_per_chain_counts():
    acc = _Acceptance(5, 1)
    acc.add([3])
    assert acc.final_rates(2) == (8 / 10., [8 / 10.])
    assert sorted(acc.state_record(2)) == ["accepted_count", "total_accepted", "total_iterations"]


def test_no_unmasked_spaxel_keeps_the_guards():
    acc = _Acceptance(0, 2)
    acc.add([0, 0])
    assert acc.running_rate(2) == 0. and acc.final_rates(2) == (0., [0., 0.])


def test_a_resumed_segment_goes_on_from_the_totals_of_its_state(tmp_path):
    """The state entries written after 4 iterations, fed back in (through an .npz, as
    ``resume_state=`` reads them): the segment's iteration 1 is the state's iteration 4."""
    np.savez(str(tmp_path / "s.npz"), **fresh_segment().state_record(4))
    acc = _Acceptance(5, 2, np.load(str(tmp_path / "s.npz")))
    assert (acc._acc_base, acc._it_base) == (22 - 10, 4 - 1)
    assert acc.running_rate(1) == 22 / 40.              # where the first segment ended
    acc.add([1, 2])
    assert acc.running_rate(2) == 25 / 50.
    pooled, per_chain = acc.final_rates(2)
    assert pooled == 25 / 50. and per_chain == [11 / 25., 14 / 25.]
    # ... which is the one segment of all four calls
    whole = fresh_segment()
    whole.add([1, 2])
    assert whole.final_rates(5) == (pooled, per_chain)
    record, expected = acc.state_record(2), whole.state_record(5)
    assert record["accepted_count"] == 10 + 3 and expected["accepted_count"] == 25
    for key in ("total_accepted", "total_iterations"):
        assert record[key] == expected[key]
    assert list(record["per_chain_accepted"]) == list(expected["per_chain_accepted"]) == [11, 14]


def test_a_state_of_one_segment_only_falls_back_to_its_count_and_iteration():
    acc = _Acceptance(5, 2, dict(accepted_count=22, iteration=4))
    assert (acc._acc_base, acc._it_base) == (12, 3)
    # (per chain: the even share, 11 of 20 each)
    assert acc.final_rates(1) == (22 / 40., [11 / 20., 11 / 20.])
    assert acc.state_record(1)["total_accepted"] == 22 and acc.state_record(1)["total_iterations"] == 4


def test_a_state_without_per_chain_counts_shares_the_total_evenly_and_truncates():
    acc = _Acceptance(5, 3, dict(total_accepted=50, total_iterations=4, accepted_count=7, iteration=2))
    acc.add([2, 0, 1])
    pooled, per_chain = acc.final_rates(2)
    assert pooled == 53 / 75.                           # (15 + 3 + 50 - 15) / (15 * 5)
    assert per_chain == [18 / 25., 16 / 25., 17 / 25.]   # 50 // 3 = 16 each: 2 of the 50 are lost
    record = acc.state_record(2)
    assert list(record["per_chain_accepted"]) == [18, 16, 17] and record["total_accepted"] == 53


@pytest.mark.parametrize("keep_one_in, slots", [(1, {1: 1, 3: 3, 4: 4}), (3, {1: 1, 3: 1, 4: 2})])
def test_valid_chain_slots_after_an_iteration(keep_one_in, slots):
    run = d3d.Run.__new__(d3d.Run)
    run.keep_one_in = keep_one_in
    assert {iteration: run._n_valid(iteration) for iteration in slots} == slots
