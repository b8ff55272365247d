"""GPU: step lanes — ShardedFlow.step running consecutive steps on the two lanes of ONE native flow handle (DESIGN.md 6.6;
include/higsfa.h "Step lanes"): per-lane workspace, tile-queue counters and error word over one copy of the weights, a stream
per lane.  A lane runs exactly the launches hg_flow_execute_device issues, so every comparison here is torch.equal against
flow.execute_device of the same rows on a handle that never had lanes."""
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 20
PRESET, SIDE = "U11L-128", 128
N_MAX = 16 * 33 + 5      # more 16-row tiles than one queue grab per workgroup: both lanes' tile queues advance across steps


def _flow(**kw):
    from pyfaceanalysis_amd import synth
    from pyfaceanalysis_amd.flow import Flow
    blob, _ = synth.cached_preset_blob(PRESET)
    return Flow.from_blob(blob, device=0, output_dtype=np.float32, **kw)


class _Serial(object):
    """Three different input blocks and, computed once per (block, rows) and never changed, what flow.execute_device gives for
    their first rows on a serial handle."""

    def __init__(self):
        import torch
        from pyfaceanalysis_amd import synth
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.flow = _flow()
        self.xs = [torch.from_numpy(synth.make_subimages(N_MAX, SIDE, seed=500 + i, dtype=np.float32)).to(self.dev) for i in range(3)]
        self._want = {}
        # stands for whoever uses a step's features; never sf.stream.  The process's one shared side stream, not a new one: which
        # hardware queue a stream lands on depends on how many were created before it (sharded._side_stream), and a stream made
        # here would move the gather's stream of every later test in this process to another queue
        from pyfaceanalysis_amd.sharded import _side_stream
        self.consumer = _side_stream(torch, self.dev)

    def keep(self, sf, y, kept, tag):
        """What a consumer does with a step it does not wait for on the host: its own stream waits for the step's event and copies
        the features there.  sf.stream is never made to wait for a step, so the next step's "ready" is not behind this one and
        the two are in flight together.  The caller makes sf.stream wait for the copy of step i - 2 (the event kept here) before it
        enqueues step i, which rewrites that buffer: "valid only until step i + 2"."""
        torch = self.torch
        self.consumer.wait_event(sf.done_event())
        with torch.cuda.stream(self.consumer):
            c = y.clone()
            ev = torch.cuda.Event()
            ev.record(self.consumer)
        kept.append((tag, c, ev))

    def want(self, block, n, flow=None):
        key = (block, n, id(flow))
        if key not in self._want:
            torch = self.torch
            y = torch.zeros((n, K), dtype=torch.float32, device=self.dev)
            x = self.xs[block]
            (flow or self.flow).execute_device(x.data_ptr(), np.float32, n, x.shape[1], y.data_ptr(), np.float32, K, K)
            torch.cuda.synchronize(self.dev)
            self._want[key] = y
        return self._want[key]


@pytest.fixture(scope="module")
def serial(native_lib):
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    s = _Serial()
    yield s
    s.flow.close()


@pytest.fixture(scope="module")
def laned(native_lib):
    """One flow whose handle has two lanes, shared by the tests that do not close or grow it."""
    flow = _flow()
    yield flow
    flow.close()


@pytest.mark.parametrize("n", [48, 1, 17, N_MAX])
def test_same_bits_as_serial(serial, laned, n):
    """7 steps over three blocks in rotation: a lane that read the other lane's workspace or queue counters, or a stale buffer,
    cannot pass.  Odd steps are compared after their own done event, even ones after wait() (one step at a time); then 7 more
    steps with nothing waited for on the host and nothing that makes sf.stream wait for a step: step i + 1 is enqueued, and free
    to run, while step i does, and each step's features are copied on a consumer stream behind its done event (_Serial.keep)."""
    import torch
    from pyfaceanalysis_amd.sharded import ShardedFlow
    sf = ShardedFlow.for_flow(laned, K, n, serial.dev, collective=False)
    assert sf.lanes == 2 and laned.lanes() == 2 and serial.flow.lanes() == 1
    for i in range(7):
        y = sf.step(serial.xs[i % 3][:n])
        assert y.data_ptr() == sf.ys[i & 1].data_ptr()
        if i & 1:
            sf.done_event(i).synchronize()
            assert sf.done_event(i).query()
        else:
            sf.wait()
        assert torch.equal(y, serial.want(i % 3, n)), "step %d" % i
    kept = []
    for i in range(7, 14):
        if len(kept) >= 2:
            sf.stream.wait_event(kept[-2][2])
        y = sf.step(serial.xs[i % 3][:n])
        serial.keep(sf, y, kept, i)
    sf.wait()
    for i, y, _ in kept:
        assert torch.equal(y, serial.want(i % 3, n)), "step %d (not waited for)" % i
    with pytest.raises(ValueError):
        sf.done_event(3)
    laned.check_errors()


def test_buffer_reuse_zeroes_stale_rows(serial, laned):
    """48 rows, then 20 and 20: the third step reuses the first one's buffer, whose rows 20..47 must read zero — the zero_() on
    sf.stream is ordered behind lane 0's first step (the join) and in front of its second (the ready event)."""
    import torch
    from pyfaceanalysis_amd.sharded import ShardedFlow
    sf = ShardedFlow.for_flow(laned, K, 48, serial.dev, collective=False)
    assert sf.lanes == 2
    y0 = sf.step(serial.xs[0][:48])
    y1 = sf.step(serial.xs[1][:20])
    y2 = sf.step(serial.xs[2][:20])
    sf.wait()
    assert y2.data_ptr() == y0.data_ptr() and tuple(y2.shape) == (48, K)
    assert torch.equal(y2[:20], serial.want(2, 20))
    assert not bool(y2[20:].any())
    assert torch.equal(y1[:20], serial.want(1, 20)) and not bool(y1[20:].any())


def test_growing_a_lane_with_steps_in_flight(serial):
    """reserve(16), then steps of 16, 400, 16, 400 rows on lanes 0, 1, 0, 1 with nothing waited for: lane 1 has to grow while lane
    0's step may still run (growing waits for the lane's own last step; freeing the old buffers then drains the device, so the
    growth itself is not concurrent with the other lane — what is checked is that all four steps are right and the handle's
    bookkeeping holds).  Straight through the flow's lane entry points, each step into a buffer of its own, all "ready" on one
    stream that never waits for a step."""
    import torch
    flow = _flow()
    assert flow.set_lanes(2)
    flow.reserve(16)
    ws0 = flow.info().workspace_bytes
    st = torch.cuda.current_stream(serial.dev)
    sizes = (16, 400, 16, 400)
    ys = [torch.zeros((m, K), dtype=torch.float32, device=serial.dev) for m in sizes]
    torch.cuda.synchronize(serial.dev)
    for i, m in enumerate(sizes):
        x = serial.xs[i % 3]
        flow.step_lane_device(i & 1, x.data_ptr(), np.float32, m, x.shape[1], ys[i].data_ptr(), np.float32, K, K,
                              ready_stream=st.cuda_stream)
    torch.cuda.synchronize(serial.dev)
    for i, m in enumerate(sizes):
        assert torch.equal(ys[i], serial.want(i % 3, m)), "step %d (%d rows)" % (i, m)
    assert flow.info().workspace_bytes > ws0      # lane 1 grew; the figure is the sum over the lanes
    flow.check_errors()
    flow.close()


def test_fallbacks_stay_serial(serial, monkeypatch):
    """HIGSFA_STEP_LANES=1 and a plan that keeps one set of state (the generic plan) take the serial path: same features as
    execute_device on the same handle, ordered on sf.stream itself, and done_event() still answers (None: nothing to wait for)."""
    import torch
    from pyfaceanalysis_amd import _capi
    from pyfaceanalysis_amd.sharded import ShardedFlow
    n = 48
    monkeypatch.setenv("HIGSFA_STEP_LANES", "1")
    flow = _flow()
    sf = ShardedFlow.for_flow(flow, K, n, serial.dev, collective=False)
    assert sf.lanes == 1 and flow.lanes() == 1
    for i in range(3):
        y = sf.step(serial.xs[i % 3][:n])
        assert sf.done_event() is None
        assert torch.equal(y, serial.want(i % 3, n))      # (torch.equal runs on sf.stream: the serial path orders the features there)
    sf.wait()
    assert sf.done_event(sf._n - 2) is None      # still answers for the two most recent steps, as documented for the serial path
    flow.close()
    monkeypatch.delenv("HIGSFA_STEP_LANES")
    gen = _flow(force_generic=True)
    assert gen.info().plan_kind == _capi.HG_PLAN_GENERIC
    assert not gen.set_lanes(2) and gen.lanes() == 1
    sf = ShardedFlow.for_flow(gen, K, n, serial.dev, collective=False)
    assert sf.lanes == 1
    for i in range(3):
        y = sf.step(serial.xs[i % 3][:n])
        assert sf.done_event() is None
        assert torch.equal(y, serial.want(i % 3, n, flow=gen))
    sf.wait()
    gen.close()


def test_close_with_steps_in_flight_and_shared_lane_streams(serial, laned):
    """flow.close() straight after two un-waited steps waits for both lanes itself; the lane streams belong to the device, not to
    a flow: every ShardedFlow on it gets the same pair."""
    import ctypes as C
    import torch
    from pyfaceanalysis_amd import _capi
    from pyfaceanalysis_amd.sharded import ShardedFlow
    flow = _flow()
    sf = ShardedFlow.for_flow(flow, K, N_MAX, serial.dev, collective=False)
    assert sf.lanes == 2
    ids = list(sf.lane_stream_ids)
    assert len(set(ids)) == 2 and all(ids)
    sf.step(serial.xs[0])
    sf.step(serial.xs[1])
    flow.close()
    torch.cuda.synchronize(serial.dev)
    sf2 = ShardedFlow.for_flow(laned, K, 48, serial.dev, collective=False)
    assert sf2.lane_stream_ids == ids
    for lane in range(2):
        sid = C.c_uint64()
        _capi.check(_capi.lib().hg_lane_stream_id(0, lane, C.byref(sid)))
        assert sid.value == ids[lane]
    y = sf2.step(serial.xs[2][:48])
    sf2.wait()
    assert torch.equal(y, serial.want(2, 48))


@pytest.fixture(scope="module")
def rccl_world1(native_lib):
    import torch
    import torch.distributed as dist
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    yield dist
    dist.destroy_process_group()


@pytest.mark.parametrize("gather_stream,light", [("side", False), ("side", True), ("same", None)])
def test_world1_collective_with_lanes(rccl_world1, serial, laned, gather_stream, light):
    """The overlapped gather against a blocking one with the lanes on, on inputs that change from step to step: the hand-off to
    the gather waits for the LANE's step, and a lane's step waits for the gather that read its buffer."""
    import torch
    from pyfaceanalysis_amd.sharded import ShardedFlow
    rows = 200
    sf = ShardedFlow.for_flow(laned, K, rows, serial.dev, collective=True, gather_stream=gather_stream, light_events=light)
    assert sf.lanes == 2 and sf.collective and sf.world == 1
    xs = [x[:rows] for x in serial.xs]
    assert sf.verify_against_blocking_gather(xs, steps=9)
    kept = []
    for i in range(6):      # nothing waited for on the host, sf.stream never waits for a step: the consumer stream (_Serial.keep)
        if len(kept) >= 2:
            sf.stream.wait_event(kept[-2][2])
        y = sf.step(xs[i % 3])
        serial.keep(sf, y, kept, i)
    sf.wait()
    for i, y, _ in kept:
        assert torch.equal(y, serial.want(i % 3, rows)), "step %d" % i
    sf.close()
