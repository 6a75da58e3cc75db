"""Pipelined scan-path calls on two lanes (csrc/ls_api.hip, lane_begin): consecutive LS_FLAG_PIPELINE calls that
are one launch each go to the handle's two internal streams in turn, the selection of a lane's launch rides on
that lane's next launch. Nothing here is a timing assert: every comparison is `array_equal` against the SAME
queries served by synchronous `search_device` calls on the same handle (exact when they return)."""

import numpy as np
import pytest

from lean_explore_amd.index import FlatIPIndex
from tests import helpers as H

pytestmark = pytest.mark.gpu

LANES_OPTION = 24    # debug option: 1 (default) two lanes for corpora of 240 MiB and more, 2 for every size, 0 the one-stream pipeline
LANE_LAUNCHES = 35   # debug counter: launches that went to a lane
LAUNCHES = 11        # debug counter: kernel launches queued by searches
SERVED_AGAIN = 25    # debug counter: queries repaired at check


def sync_rows(ix, tq, k, nq=1):
    """The queries of tq, nq per call, through synchronous device calls: [(scores, indices)] per call."""
    return [ix.search_device(tq[j:j + nq], k) for j in range(0, tq.shape[0], nq)]


def assert_same(got, want):
    import torch

    assert len(got) == len(want)
    for j, ((Dg, Ig), (Dw, Iw)) in enumerate(zip(got, want)):
        assert torch.equal(Dg, Dw) and torch.equal(Ig, Iw), f"call {j} differs from the synchronous call"


@pytest.fixture(scope="module")
def headline():
    import torch

    c = H.gauss(101, 200_000, 384)
    ix = FlatIPIndex.from_array(c)
    tq = torch.from_numpy(H.gauss(102, 300, 384)).cuda()
    yield ix, tq
    ix.close()


def test_300_calls_cross_the_self_check(headline):
    ix, tq = headline
    before = ix.debug_counter(LANE_LAUNCHES)
    outs = [ix.search_device(tq[j:j + 1], 50, pipeline=True) for j in range(300)]  # (own output rows per call)
    ix.check()
    assert ix.debug_counter(LANE_LAUNCHES) == before + 300
    assert_same(outs, sync_rows(ix, tq, 50))


def test_k_mix(headline):
    ix, tq = headline
    ks = [10, 50, 50, 7, 300, 50] * 3
    outs = [ix.search_device(tq[j:j + 1], k, pipeline=True) for j, k in enumerate(ks)]
    ix.check()
    assert_same(outs, [ix.search_device(tq[j:j + 1], k) for j, k in enumerate(ks)])


@pytest.mark.parametrize("nq", [8, 32])
def test_several_queries_per_call(headline, nq):
    ix, tq = headline
    before = ix.debug_counter(LANE_LAUNCHES)
    outs = [ix.search_device(tq[j:j + nq], 50, pipeline=True) for j in range(0, 9 * nq, nq)]
    ix.check()
    assert ix.debug_counter(LANE_LAUNCHES) == before + 9
    assert_same(outs, sync_rows(ix, tq[:9 * nq], 50, nq))


def test_long_rows_large_k():
    import torch

    c = H.gauss(103, 100_000, 1024)
    ix = FlatIPIndex.from_array(c)
    tq = torch.from_numpy(H.gauss(104, 12, 1024)).cuda()
    outs = [ix.search_device(tq[j:j + 1], 1000, pipeline=True) for j in range(12)]
    ix.check()
    assert ix.debug_counter(LANE_LAUNCHES) == 12
    assert_same(outs, sync_rows(ix, tq, 1000))
    ix.close()


def test_fp16_index():
    import torch

    c = H.gauss(105, 400_000, 384)  # (307 MB of fp16 rows: past the size from which launches take the lanes)
    ix = FlatIPIndex.from_array(c, dtype="f16")
    tq = torch.from_numpy(H.gauss(106, 20, 384)).cuda()
    outs = [ix.search_device(tq[j:j + 1], 50, pipeline=True) for j in range(20)]
    ix.check()
    assert ix.debug_counter(LANE_LAUNCHES) == 20
    assert_same(outs, sync_rows(ix, tq, 50))
    ix.close()


def test_short_and_empty_pipelines(headline):
    ix, tq = headline
    want = sync_rows(ix, tq[:3], 50)
    ix.check()  # nothing queued
    ix.check()  # ... twice
    for calls in (1, 2, 3):
        outs = [ix.search_device(tq[j:j + 1], 50, pipeline=True) for j in range(calls)]
        ix.check()
        assert_same(outs, want[:calls])
    ix.check()
    ix.check()


def test_query_buffer_is_free_once_the_callers_stream_has_passed_the_call(headline):
    """One device query buffer, overwritten on the caller's stream between consecutive pipelined calls."""
    ix, tq = headline
    buf = tq[:1].clone()
    outs = []
    for j in range(40):
        buf.copy_(tq[j:j + 1])
        outs.append(ix.search_device(buf, 50, pipeline=True))
    buf.zero_()
    ix.check()
    assert_same(outs, sync_rows(ix, tq[:40], 50))


def test_launch_starts_after_the_callers_stream(headline):
    """On a non-default stream the query is written behind a long-running op queued just before the call."""
    import torch

    ix, tq = headline
    want = sync_rows(ix, tq[:6], 50)
    s1 = torch.cuda.Stream()
    big = torch.randn(8192, 8192, device="cuda")
    buf = torch.zeros_like(tq[:6])
    torch.cuda.synchronize()
    outs = []
    with torch.cuda.stream(s1):
        for j in range(6):
            big2 = big @ big  # (milliseconds: a launch that did not wait would read zeros)
            buf[j:j + 1].copy_(tq[j:j + 1])
            outs.append(ix.search_device(buf[j:j + 1], 50, pipeline=True, stream=s1))
        ix.check(s1)
    torch.cuda.synchronize()
    del big2
    assert_same(outs, want)


def test_stream_switch_async_and_host_calls_between_pipelined_calls(headline):
    import torch

    ix, tq = headline
    want = sync_rows(ix, tq[:8], 20)
    want3 = ix.search_device(tq[2:5], 20)
    qs = tq.cpu().numpy()
    s2 = torch.cuda.Stream()
    a = ix.search_device(tq[0:1], 20, pipeline=True)
    a1 = ix.search_device(tq[1:2], 20, pipeline=True)
    b = ix.search_device(tq[2:3], 20, pipeline=True, stream=s2)  # another caller's stream mid-pipeline
    b1 = ix.search_device(tq[3:4], 20, pipeline=True, stream=s2)
    cc = ix.search_device(tq[2:5], 20, asynchronous=True)         # ordered, 3 queries
    e = ix.search_device(tq[5:6], 20, pipeline=True)
    d2, i2 = ix.search(qs[6:7], 20)                                # host API
    f = ix.search_device(tq[7:8], 20, pipeline=True)
    ix.check(s2)
    ix.check()
    torch.cuda.synchronize()
    assert_same([a, a1, b, b1, e, f], [want[0], want[1], want[2], want[3], want[5], want[7]])
    assert_same([cc], [want3])
    assert np.array_equal(d2, want[6][0].cpu().numpy()) and np.array_equal(i2, want[6][1].cpu().numpy())


def test_repairs_under_lanes():
    """A clustered (sorted) corpus and k' = 1: the selections cannot prove their keys complete and the queries are
    served again at check - into the rows of the call that asked."""
    import torch

    c = H.gauss(3, 200_000, 384)
    q = H.gauss(4, 12, 384)
    c = np.ascontiguousarray(c[np.argsort(c @ q[0])])
    ix = FlatIPIndex.from_array(c)
    tq = torch.from_numpy(q).cuda()
    want1 = sync_rows(ix, tq, 64)
    want4 = sync_rows(ix, tq, 64, 4)
    ix.debug_option(0, 1)
    before, lanes = ix.debug_counter(SERVED_AGAIN), ix.debug_counter(LANE_LAUNCHES)
    outs1 = [ix.search_device(tq[j:j + 1], 64, pipeline=True) for j in range(12)]
    outs4 = [ix.search_device(tq[j:j + 4], 64, pipeline=True) for j in range(0, 12, 4)]
    ix.check()
    assert ix.debug_counter(SERVED_AGAIN) >= before + 4
    assert ix.debug_counter(LANE_LAUNCHES) == lanes + 15
    assert_same(outs1, want1)
    assert_same(outs4, want4)
    # more launches than kept-query slots between two checks, every one of them in need of a repair
    outs = [ix.search_device(tq[j % 12:j % 12 + 1], 64, pipeline=True) for j in range(300)]
    ix.check()
    assert_same(outs, [want1[j % 12] for j in range(300)])
    ix.close()


def test_option_off_same_bits_and_no_lane_launches(headline):
    ix, tq = headline
    on = [ix.search_device(tq[j:j + 1], 50, pipeline=True) for j in range(10)]
    on8 = [ix.search_device(tq[j:j + 8], 50, pipeline=True) for j in range(0, 32, 8)]
    ix.check()
    ix.debug_option(LANES_OPTION, 0)
    try:
        before = ix.debug_counter(LANE_LAUNCHES)
        off = [ix.search_device(tq[j:j + 1], 50, pipeline=True) for j in range(10)]
        off8 = [ix.search_device(tq[j:j + 8], 50, pipeline=True) for j in range(0, 32, 8)]
        ix.check()
        assert ix.debug_counter(LANE_LAUNCHES) == before
    finally:
        ix.debug_option(LANES_OPTION, 1)
    lanes = ix.debug_counter(LANE_LAUNCHES)
    again = [ix.search_device(tq[j:j + 1], 50, pipeline=True) for j in range(10)]
    ix.check()
    assert ix.debug_counter(LANE_LAUNCHES) == lanes + 10
    assert_same(on, off)
    assert_same(on8, off8)
    assert_same(again, off)


def test_profiling_keeps_pipelined_launches_on_one_stream(headline):
    ix, tq = headline
    want = sync_rows(ix, tq[:6], 50)
    ix.set_profiling(True)
    try:
        before = ix.debug_counter(LANE_LAUNCHES)
        outs = [ix.search_device(tq[j:j + 1], 50, pipeline=True) for j in range(6)]
        ix.check()
        assert ix.debug_counter(LANE_LAUNCHES) == before
        assert ix.last_kernel_ms()[0] > 0
    finally:
        ix.set_profiling(False)
    assert_same(outs, want)


@pytest.mark.parametrize("nq", [1, 8])
def test_one_launch_per_call_and_at_most_two_per_check(headline, nq):
    ix, tq = headline
    ix.check()
    for calls in (1, 2, 5, 40):
        before = ix.debug_counter(LAUNCHES)
        for j in range(calls):
            ix.search_device(tq[j:j + nq], 50, pipeline=True)
        queued = ix.debug_counter(LAUNCHES)
        assert queued == before + calls
        ix.check()
        assert queued <= ix.debug_counter(LAUNCHES) <= queued + 2


def test_close_and_add_with_launches_pending():
    import torch

    c = H.gauss(107, 30_000, 384)
    more = H.gauss(108, 5_000, 384)
    tq = torch.from_numpy(H.gauss(109, 8, 384)).cuda()
    ix = FlatIPIndex.from_array(c)  # 46 MB: a pass shorter than a lane call's queueing work stays on one stream
    outs = [ix.search_device(tq[j:j + 1], 20, pipeline=True) for j in range(5)]
    ix.check()
    assert ix.debug_counter(LANE_LAUNCHES) == 0
    ix.close()
    for _ in range(3):  # create, queue on both lanes, close without a check
        ix = FlatIPIndex.from_array(c)
        ix.debug_option(LANES_OPTION, 2)
        outs = [ix.search_device(tq[j:j + 1], 20, pipeline=True) for j in range(5)]
        assert ix.debug_counter(LANE_LAUNCHES) == 5
        ix.close()
        torch.cuda.synchronize()
        del outs
    ix = FlatIPIndex.from_array(c)
    ix.debug_option(LANES_OPTION, 2)
    want = sync_rows(ix, tq, 20)
    outs = [ix.search_device(tq[j:j + 1], 20, pipeline=True) for j in range(8)]
    assert ix.debug_counter(LANE_LAUNCHES) == 8
    ix.add(more)  # synchronises the handle first: what was queued is final
    torch.cuda.synchronize()
    assert_same(outs, want)
    assert ix.ntotal == 35_000
    both = FlatIPIndex.from_array(np.concatenate([c, more]))
    outs = [ix.search_device(tq[j:j + 1], 20, pipeline=True) for j in range(8)]
    ix.check()
    assert_same(outs, sync_rows(both, tq, 20))
    both.close()
    ix.close()
