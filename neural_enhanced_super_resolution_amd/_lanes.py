"""RealESRGANer(devices=[...]): the entries of `devices` as lanes -- (device, occurrence among the entries with the same index, which
picks the context replicas, stream) -- and the sequence both multi-device routes follow (run_shares).  `streams`: RealESRGANer._streams."""
import os

import numpy as np
import torch


def parse_devices(devices, count):
    """RealESRGANer's ``devices=`` keyword -> list of CUDA device indices, or None for the one-device wrapper.  With
    ``devices=None`` the NESR_DEVICES environment variable (comma-separated indices, e.g. "0,1,2,3") is read instead, so
    callers that cannot pass the keyword opt in from outside; unset or empty means None.  Repeated indices are allowed
    (several contexts on one device).  An empty list, a non-integer or an index outside [0, count) raises ValueError."""
    source = "devices"
    if devices is None:
        devices = os.environ.get("NESR_DEVICES", "").strip()
        if not devices:
            return None
        source = "NESR_DEVICES"
    if isinstance(devices, str):
        try:
            devices = [int(v) for v in devices.split(",")]
        except ValueError:
            raise ValueError(f"{source}={devices!r}: expected comma-separated CUDA device indices") from None
    out = []
    for d in devices:
        if isinstance(d, bool) or not isinstance(d, (int, np.integer)):
            raise ValueError(f"{source}: {d!r} is not a CUDA device index")
        out.append(int(d))
    if not out:
        raise ValueError(f"{source}: the device list is empty")
    for d in out:
        if d < 0 or d >= count:
            raise ValueError(f"{source}: device {d} does not exist ({count} visible)")
    return out


def lane_slots(devices):
    """[(device, occurrence)] per entry of `devices`: occurrence = earlier entries with the same index."""
    return [(torch.device("cuda", d), devices[:j].count(d)) for j, d in enumerate(devices)]


def lanes(devices, streams, home):
    """([(device, occurrence, stream)] per entry, the gather stream on `home`); the first entry runs on the caller's stream."""
    out = []
    for j, (dev, o) in enumerate(lane_slots(devices)):
        if j and j not in streams.lane:
            streams.lane[j] = torch.cuda.Stream(device=dev)
        out.append((dev, o, streams.lane[j] if j else torch.cuda.current_stream(dev)))
    if streams.gather is None:
        streams.gather = torch.cuda.Stream(device=home)
    return out, streams.gather


def send_home(flat, lane_stream, gather, items, dst):
    """`flat` (contiguous, on a lane's device, written on `lane_stream`) -> one device-to-device copy to the first device
    on `gather`, whose slices [offset, offset + numel) are then pasted into dst[index] (items: [(offset, shape, index)]).
    Every tensor involved is used on the stream it was allocated on, so none has to outlive the call."""
    with torch.cuda.stream(gather):
        with torch.cuda.stream(lane_stream):
            buf = torch.empty(flat.shape, dtype=flat.dtype, device=dst.device)
            buf.copy_(flat, non_blocking=True)      # on the lane's stream, after its tiles; `gather` waits for it
        for off, shape, index in items:
            n = int(np.prod(shape))
            dst[index] = buf[off:off + n].view(shape)


def run_shares(lanes, shares, gather, dst, srcs, copy, run_share):
    """One frame's shares on their lanes, the results into `dst` (on the first device, made on its current stream, which `gather`
    waits for, as every used lane does for its device's).  `srcs`, the caller's {device index: (source, event or None)}, gains
    ``copy(dev, st)`` and an event behind it for each device it lacks.  Per lane, after that event, ``run_share(dev, occurrence,
    st, share, src)`` returns None (it wrote into `dst`) or ``(flat, items)`` for send_home.  Last, the current streams wait."""
    home = dst.device
    used = [(lane, share) for lane, share in zip(lanes, shares) if share]
    gather.wait_stream(torch.cuda.current_stream(home))
    for (dev, _, st), _ in used:
        if st != torch.cuda.current_stream(dev):
            st.wait_stream(torch.cuda.current_stream(dev))   # dst; the lane's replicas may still be in use there
    for (dev, _, st), _ in used:
        if dev.index not in srcs:
            srcs[dev.index] = (copy(dev, st), torch.cuda.Event())
            srcs[dev.index][1].record(st)
    for (dev, o, st), share in used:
        src, ev = srcs[dev.index]
        with torch.cuda.device(dev), torch.cuda.stream(st):
            if ev is not None:
                st.wait_event(ev)                   # every lane of the device, not only the one the copy was made for
            sent = run_share(dev, o, st, share, src)
            if sent is not None:
                send_home(sent[0], st, gather, sent[1], dst)
    for dev, _, st in lanes:                        # every device's current stream waits for the lanes on it ...
        if st != torch.cuda.current_stream(dev):
            torch.cuda.current_stream(dev).wait_stream(st)
    torch.cuda.current_stream(home).wait_stream(gather)   # ... and the first device's for the copies home
