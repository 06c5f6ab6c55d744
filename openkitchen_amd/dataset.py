"""Laser-scan dataset writer: the text files the reference's data collectors produce,
`<dir>/laser2d_<track>_<ctr>.txt` = one "hit.x hit.y" line per ray (Agent::sensor_hits_, the "robot frame" hit points)
followed by "throttle steering" without a trailing newline (FieldNavigators/collect_data/collect_data_random.cpp:65-96,
MeasurementMode::Laser2d), written from the batched environment: one file per agent and recorded step, numbered in
agent order within a step.  Values are formatted like `std::ostream << float` (six significant digits, %g).

Off the hot path: this reads the device buffers back once per recorded step.

Also here: `BirdseyeWriter` for MeasurementMode::BirdseyeView (collect_data_random.cpp:72-82): `birdseye_<track>_<ctr>.txt`
holding "throttle steering" and `birdseye_<track>_<ctr>.png` beside it, and `Laser2dWriter.save_recorded` /
`BirdseyeWriter.save_recorded`, which write from the tensors openkitchen_amd/demonstrations.py records.
"""
import os
import struct
import zlib

import numpy as np

from . import _capi as capi


def _fmt(x):
    return "%g" % float(x)


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


class Laser2dWriter:
    def __init__(self, directory, track_name):
        self.directory, self.track_name, self.ctr = directory, track_name, 0
        os.makedirs(directory, exist_ok=True)  # collect_data_random.cpp:46-49

    def path(self, ctr):
        return os.path.join(self.directory, "laser2d_%s_%d.txt" % (self.track_name, ctr))

    def write_sample(self, hits_xy, throttle, steering):
        """One DataCollectorAgent::saveMeasurement call; hits_xy is [R, 2]."""
        lines = ["%s %s\n" % (_fmt(x), _fmt(y)) for x, y in hits_xy]
        with open(self.path(self.ctr), "w") as f:
            f.write("".join(lines) + "%s %s" % (_fmt(throttle), _fmt(steering)))
        self.ctr += 1

    def save(self, env, agents=None, skip_crashed=True):
        """Records the current observation and action of `agents` (default: all) of a BatchedEnvironment; crashed
        agents are skipped: the reference only records inside `while (... && !agent->crashed_)` (collect_data_random.cpp:177-183).  Returns the number
        of files written."""
        hits = env.hits()
        thr, steer = env.get(capi.F_THROTTLE), env.get(capi.F_STEER)
        crashed = env.get(capi.F_CRASHED)
        idx = range(env.N) if agents is None else agents
        n = 0
        for a in idx:
            if skip_crashed and crashed[a]:
                continue
            self.write_sample(hits[a], thr[a], steer[a])
            n += 1
        return n

    def save_recorded(self, actions, rel_xy, alive=None):
        """Writes the samples of recorded tensors (actions [T,N,2], rel_xy [T,N,R,2], alive [T,N] or None; torch or numpy), step by
        step and in agent order within a step, skipping entries with alive == 0.  Returns the number of files written."""
        actions, rel_xy = _host(actions), _host(rel_xy)
        alive = None if alive is None else _host(alive)
        n = 0
        for t in range(actions.shape[0]):
            for a in range(actions.shape[1]):
                if alive is not None and not alive[t, a]:
                    continue
                self.write_sample(rel_xy[t, a], actions[t, a, 0], actions[t, a, 1])
                n += 1
        return n


def encode_png(frame):
    """A frame [H, W, 4] (RGBA), [H, W, 3] (RGB) or [H, W] (grey) of uint8 as PNG bytes: filter 0 on every row, deflated
    with zlib."""
    frame = np.ascontiguousarray(frame, dtype=np.uint8)
    if frame.ndim == 2:
        frame = frame[:, :, None]
    h, w, c = frame.shape
    color = {1: 0, 3: 2, 4: 6}[c]
    raw = np.concatenate([np.zeros((h, 1), dtype=np.uint8), frame.reshape(h, w * c)], axis=1).tobytes()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, color, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def decode_png(data):
    """Inverse of encode_png (8-bit, filter 0 only): the frame as [H, W, C] uint8."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == (zlib.crc32(tag + body) & 0xFFFFFFFF)
        if tag == b"IHDR":
            w, h, depth, color = struct.unpack(">IIBB", body[:10])
            assert depth == 8
            c = {0: 1, 2: 3, 6: 4}[color]
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + w * c)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(h, w, c).copy()


class BirdseyeWriter:
    """MeasurementMode::BirdseyeView of DataCollectorAgent::saveMeasurement (collect_data_random.cpp:72-82)."""

    def __init__(self, directory, track_name):
        self.directory, self.track_name, self.ctr = directory, track_name, 0
        os.makedirs(directory, exist_ok=True)

    def path(self, ctr, ext=".txt"):
        return os.path.join(self.directory, "birdseye_%s_%d%s" % (self.track_name, ctr, ext))

    def write_sample(self, frame, throttle, steering):
        with open(self.path(self.ctr), "w") as f:
            f.write("%s %s" % (_fmt(throttle), _fmt(steering)))
        with open(self.path(self.ctr, ".png"), "wb") as f:
            f.write(encode_png(frame))
        self.ctr += 1

    def save_recorded(self, actions, frames, alive=None):
        """actions [T,N,2], frames [T,N,H,W,4] or [T,N,H,W], alive [T,N] or None; entries with alive == 0 are skipped."""
        actions, frames = _host(actions), _host(frames)
        alive = None if alive is None else _host(alive)
        n = 0
        for t in range(actions.shape[0]):
            for a in range(actions.shape[1]):
                if alive is not None and not alive[t, a]:
                    continue
                self.write_sample(frames[t, a], actions[t, a, 0], actions[t, a, 1])
                n += 1
        return n


def read_sample(path):
    """Parses one laser2d file back into (hits [R, 2] float32, throttle, steering)."""
    rows = [ln.split() for ln in open(path).read().split("\n") if ln.strip()]
    hits = np.array(rows[:-1], dtype=np.float32).reshape(-1, 2)
    return hits, float(rows[-1][0]), float(rows[-1][1])
