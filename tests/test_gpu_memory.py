"""-m gpu: a context gives back all the device memory it took.  Every resource of a context releases itself when the context is
destroyed (csrc/device/resources.hpp, context.hpp); nothing else in the suite would see a buffer that is forgotten there, or one that
adypt_set_frames_in_flight leaves behind when it replaces the ray queues."""
import time

import pytest

pytestmark = pytest.mark.gpu

from adypt_amd import api, scenes  # noqa: E402

# What the free memory of the device may differ by between the end of cycle 2 and the end of cycle 10.
# Measured with this very loop on the commit before the owners existed (free lists kept by hand, no leak known): free memory fell by 182.5 MB in
# cycle 1 and by 16.8 MB in cycle 2 (the runtime's own pools filling), then read 308 356 841 472 bytes after every one of cycles 2 .. 10: drift 0.
# The runtime hands device memory out in granules of 2 MiB (there, hipMalloc of 1 MiB moved the free memory by 2 MiB, of 2 MiB + 1 by 4 MiB, and
# allocations of up to 4 KiB not at all).  The bound is that drift plus one granule.  With the owners the same loop read the same numbers.
# At 96 x 64 a context owns 6 blocks = 6144 local pixels and has 128 frames in flight, so ONE ray-queue array is 16 B x 128 x 6144 = 12.6 MB:
# a single array forgotten in a single cycle is 6 x the bound, one forgotten in every cycle 8 x 12.6 MB.
PARENT_DRIFT_BYTES = 0
GRANULE_BYTES = 2 << 20
BOUND_BYTES = PARENT_DRIFT_BYTES + GRANULE_BYTES
ONE_QUEUE_ARRAY_BYTES = 16 * 128 * 6144


def _free_bytes():
    free = api.device_free_bytes(0)
    if free is None:  # (next to torch's copy of the runtime the helper may not answer: torch reports the same quantity)
        import torch
        free = torch.cuda.mem_get_info(0)[0]
    return int(free)


def _cycle(cache):
    """Everything a context can own: two replacements of the ray queues and every buffer that is made on first use."""
    spec = scenes.make_scene("tiny0", cache, width=96, height=64, pt={"maxBounce": 4, "stackSize": 16})
    inst = api.Instance()
    assert inst.InitializeFromFile(spec.config_path, shift_seed=7), api.InstanceConfig.last_error()
    p = inst.m_path_tracer
    assert p.GetFramesInFlight() == 128
    p.Trace(True, 3)
    p.SetFramesInFlight(16)
    p.Trace(True, 2)
    p.SetFramesInFlight(128)
    p.SetInstrumentation(timing=True, audit=True)  # the pool of timing events and the audit's bitmaps
    p.Trace(True, 2)
    p.SetInstrumentation()  # (the bitmaps stay; the audit is not run next to sun-visibility queries, which it does not know)
    p.SetSunVisibility(True)
    p.Trace(True, 2)  # the queries ride in the ray queues
    p.SetFusedBounces(False)
    p.Trace(True, 2)  # a launch per bounce: the sun-visibility queue of its own
    p.ReadDisplay()
    p.ReadHits()
    p.destroy()


def test_contexts_give_their_device_memory_back(scene_cache):
    assert ONE_QUEUE_ARRAY_BYTES >= 4 * BOUND_BYTES
    a = _free_bytes()
    time.sleep(1.0)
    b = _free_bytes()
    if abs(a - b) > BOUND_BYTES:
        pytest.skip("another process is changing the device's free memory (%d bytes within a second)" % abs(a - b))
    after = {}
    for cycle in range(1, 11):
        _cycle(scene_cache)
        after[cycle] = _free_bytes()
    print("free bytes after each cycle:", after, "| drift 2 -> 10:", after[2] - after[10])
    assert abs(after[2] - after[10]) <= BOUND_BYTES, after
