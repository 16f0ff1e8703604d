"""ContextPool without a GPU: the calls it makes on the library, in order, for every rule of its docstring.  The library is a
fake that records (function, handle, args); create / upload hand out counters; the device guard records the device it is for."""
import contextlib

import pytest

from neural_enhanced_super_resolution_amd import _contexts
from neural_enhanced_super_resolution_amd._contexts import ContextPool

F32, BF16 = 3, 1
CONC = "nesr_set_concurrent"


class Recorder:
    """lib, create and upload of one pool; `log` is what they were asked, take() hands it over and starts afresh."""

    def __init__(self):
        self.log = []
        self.made = 0

    def __getattr__(self, name):            # the library: every entry records and succeeds
        def entry(handle, *args):
            self.log.append((name, handle, args))
            return 0
        return entry

    def create(self, index, code):
        self.made += 1
        handle = f"h{self.made}"
        self.log.append(("create", handle, (index, code)))
        return handle

    def upload(self, handle):
        self.log.append(("upload", handle, ()))

    def take(self):
        out, self.log = self.log, []
        return out


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()

    @contextlib.contextmanager
    def guard(index):
        r.log.append(("guard", None, (index,)))
        yield

    monkeypatch.setattr(_contexts, "_device_guard", guard)
    return r


@pytest.fixture
def pool(rec):
    p = ContextPool(rec.create, rec.upload, lib=rec)
    p.set("nesr_set_fused", 0)              # before any context exists: no call, applied at creation
    p.set("nesr_set_upconv", 1)
    assert rec.take() == []
    return p


def new(handle, index, code=F32):
    """What creating one context asks: create, upload, then every recorded setting in insertion order."""
    return [("create", handle, (index, code)), ("upload", handle, ()), ("nesr_set_fused", handle, (0,)), ("nesr_set_upconv", handle, (1,))]


def test_first_and_second_request(pool, rec):
    assert pool.home is None and pool.handles() == [] and pool.devices() == [] and pool.handle(0, 0) is None
    assert pool.get(0, 0, F32) == "h1"
    assert rec.take() == new("h1", 0)
    assert (pool.home, pool.code) == (0, F32)
    assert pool.get(0, 0, F32) == "h1"
    assert rec.take() == []


def test_home_replica_marks_every_home_context_concurrent(pool, rec):
    pool.get(0, 0, F32)
    rec.take()
    assert pool.get(0, 1, F32) == "h2"
    assert rec.take() == new("h2", 0) + [(CONC, "h1", (1,)), (CONC, "h2", (1,))]
    assert pool.get(0, 1, F32) == "h2" and rec.take() == []
    assert pool.get(0, 5, F32) == "h3"
    assert rec.take() == new("h3", 0) + [(CONC, h, (1,)) for h in ("h1", "h2", "h3")]


def test_replica_first_settles_slot_0(pool, rec):
    assert pool.get(2, 1, F32) == "h2"
    assert rec.take() == new("h1", 2) + new("h2", 2) + [(CONC, "h1", (1,)), (CONC, "h2", (1,))]
    assert pool.home == 2 and pool.handle(2, 0) == "h1"


def test_dirty_reuploads_slot_0_in_place_and_drops_the_rest(pool, rec):
    pool.get(0, 0, F32)
    pool.get(0, 1, F32)
    pool.get(1, 0, F32)
    rec.take()
    pool.mark_dirty()
    assert rec.take() == []
    assert pool.get(0, 0, F32) == "h1"                       # the same handle, one upload, the others destroyed first
    assert rec.take() == [("nesr_destroy", "h2", ()), ("nesr_destroy", "h3", ()), ("upload", "h1", ())]
    assert pool.handles() == ["h1"] and pool.handle(0, 1) is None and pool.handle(1, 0) is None
    assert pool.get(0, 1, F32) == "h4"                       # re-created lazily, with its settings
    assert rec.take() == new("h4", 0) + [(CONC, "h1", (1,)), (CONC, "h4", (1,))]
    pool.mark_dirty()
    assert pool.get(0, 1, F32) == "h5"                       # a replica request settles slot 0 first
    assert rec.take() == [("nesr_destroy", "h4", ()), ("upload", "h1", ())] + new("h5", 0) + [(CONC, "h1", (1,)), (CONC, "h5", (1,))]


def test_other_device(pool, rec):
    pool.get(0, 0, F32)
    rec.take()
    assert pool.get(1, 0, F32) == "h2"                       # home settled under its guard (nothing to do), then the context
    assert rec.take() == [("guard", None, (0,))] + new("h2", 1)
    assert pool.home == 0
    assert pool.get(1, 0, F32) == "h2"
    assert rec.take() == [("guard", None, (0,))]
    assert pool.get(1, 2, F32) == "h3"                       # two on device 1: both marked, the home's context is not
    assert rec.take() == [("guard", None, (0,))] + new("h3", 1) + [(CONC, "h2", (1,)), (CONC, "h3", (1,))]
    pool.mark_dirty()
    assert pool.get(1, 2, F32) == "h4"                       # stale weights: home re-uploaded under its guard, the rest re-made
    assert rec.take() == [("guard", None, (0,)), ("nesr_destroy", "h2", ()), ("nesr_destroy", "h3", ()), ("upload", "h1", ())] + new("h4", 1)


def test_changed_code_releases_everything(pool, rec):
    pool.get(0, 0, F32)
    pool.get(0, 1, F32)
    pool.get(1, 0, F32)
    rec.take()
    assert pool.get(1, 0, BF16) == "h4"                      # a new home, on another index, with the settings
    assert rec.take() == [("nesr_destroy", h, ()) for h in ("h1", "h2", "h3")] + new("h4", 1, BF16)
    assert (pool.home, pool.code) == (1, BF16) and pool.handles() == ["h4"]


def test_set_reaches_live_contexts_in_handles_order(pool, rec):
    pool.get(0, 0, F32)
    pool.get(1, 0, F32)
    pool.get(0, 1, F32)                                      # a home replica made after the other device's context
    pool.get(1, 1, F32)
    rec.take()
    assert pool.handles() == ["h1", "h3", "h2", "h4"]        # home slot 0, home replicas, then the other devices'
    assert pool.handles(device=1) == ["h2", "h4"] and pool.handles(device=0) == ["h1", "h3"] and pool.handles(device=7) == []
    assert pool.devices() == [0, 1]
    assert (pool.handle(0, 1), pool.handle(1, 1), pool.handle(1, 5)) == ("h3", "h4", None)
    pool.set("nesr_set_kernel_timing", True)
    assert rec.take() == [("nesr_set_kernel_timing", h, (1,)) for h in ("h1", "h3", "h2", "h4")]
    pool.set("nesr_set_fused", 1)                            # a changed value keeps its place in the replay order
    rec.take()
    assert list(pool.settings.items()) == [("nesr_set_fused", 1), ("nesr_set_upconv", 1), ("nesr_set_kernel_timing", 1)]
    pool.get(0, 2, F32)
    assert rec.take()[:5] == [("create", "h5", (0, F32)), ("upload", "h5", ()), ("nesr_set_fused", "h5", (1,)), ("nesr_set_upconv", "h5", (1,)),
                              ("nesr_set_kernel_timing", "h5", (1,))]


def test_set_concurrent_is_not_sticky(pool, rec):
    pool.get(0, 0, F32)
    pool.get(0, 1, F32)
    rec.take()
    pool.set_concurrent(False)
    assert rec.take() == [(CONC, "h1", (0,)), (CONC, "h2", (0,))]
    assert CONC not in pool.settings
    pool.get(1, 0, F32)
    assert rec.take() == [("guard", None, (0,))] + new("h3", 1)


def test_release_keeps_settings_and_is_harmless_twice(pool, rec):
    pool.get(0, 0, F32)
    pool.get(1, 0, F32)
    rec.take()
    pool.release()
    assert rec.take() == [("nesr_destroy", "h1", ()), ("nesr_destroy", "h2", ())]
    assert pool.home is None and pool.handles() == [] and pool.dirty
    pool.release()
    assert rec.take() == []
    assert pool.get(1, 0, F32) == "h3"                       # the next slot-0 context defines a new home and is told the switches
    assert rec.take() == new("h3", 1) and pool.home == 1


def test_refused_upload_leaves_nothing_behind(pool, rec):
    def refuse(handle):
        raise ValueError("weights out of range")

    pool._upload = refuse
    with pytest.raises(ValueError):
        pool.get(0, 0, F32)
    assert rec.take() == [("create", "h1", (0, F32)), ("nesr_destroy", "h1", ())]
    assert pool.home is None and pool.handles() == []
