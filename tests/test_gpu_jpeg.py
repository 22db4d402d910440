"""The frame encoder on the GPU (ray_tracer_s8_amd/frame_encoder.py, jpeg_csrc/): rtj_encode equals the restatement
tests/_jpeg_np.py in every byte of [0, total) and in the record, the output beyond total and a sentinel-filled tail past the capacity
are untouched, and the frame is read back unchanged:
1. with no scene, the corpus of the host test: 8 x 8 (one MCU, one interval, no RST), 13 x 21 and 67 x 19 (ragged both ways, 27 MCUs:
   less than a transform block), 72 x 16 at interval 1 (18 intervals: RST wraps past 7), 67 x 19 at intervals 1, 3, a row of MCUs and
   one beyond the MCU count; flat grey, uniform noise at quality 100 (stuffed 0xFF bytes and a padded last byte of 0xFF: asserted on
   the restatement by the host test and again here), a single high-frequency coefficient (ZRL), the checkerboard at quality 100 (the
   largest categories), 0 and 255 in every channel, black beside white (a DC difference of category 11); qualities 1, 50, 90, 100;
   and 264 x 264 at intervals 1 and 7 (1 089 MCUs and as many intervals: both scans pass a chunk of 1 024) and at the caller's tables;
2. overflow: a capacity one byte short and one of header_len + 1 give the flag, the true total and no write at or past the capacity;
3. the chain: FrameEncoder.encode on a FilmDisplay frame of a 96 x 54 c2 film decodes with Pillow and is the restatement's file for the
   same rgb; encode_device, record(), header, tables and bound; the retry on overflow; the refusals.
Every body runs in a child process that imports torch first.  Without the feature every test here fails: there is no rt.FrameEncoder
and no librt_jpeg.so.  No timing is asserted."""
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

_PRELUDE = r"""
import ctypes as C
import io
import math
import sys
import numpy as np
import torch                                                      # first: the libraries then bind to torch's HIP runtime
sys.path.insert(0, "tests")
import ray_tracer_s8_amd as rt
from ray_tracer_s8_amd import _jpeg_lib as jl, frame_encoder as fe, scenes
import _jpeg_np as jnp

dev = torch.device("cuda", 0)
SENTINEL, TAIL = 0xA5, 64

def upload(stream, a):
    with torch.cuda.stream(stream):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

def device_encode(lib, stream, rgb, quality, interval, capacity=None, tables=None):
    # rtj_encode into a sentinel-filled buffer of `capacity` bytes with TAIL more behind it: (the whole buffer, the record's words)
    R, W = rgb.shape[:2]
    n = C.c_uint64(0)
    jl.check("rtj_bound", lib.rtj_bound(W, R, interval, C.byref(n)))
    capacity = n.value if capacity is None else capacity
    jl.check("rtj_scratch_bytes", lib.rtj_scratch_bytes(W, R, interval, C.byref(n)))
    head = (C.c_uint8 * jl.HEADER_LEN)()
    t = None if tables is None else np.ascontiguousarray(tables, np.uint8)
    a = jl.EncodeArgs(W=W, R=R, quality=0 if tables is not None else quality, interval=interval, tables=None if t is None else t.ctypes.data)
    got = C.c_uint64(0)
    jl.check("rtj_header", lib.rtj_header(a, head, jl.HEADER_LEN, C.byref(got)))
    buf = np.full(capacity + TAIL, SENTINEL, np.uint8)
    buf[:jl.HEADER_LEN] = np.frombuffer(bytes(head), np.uint8)
    d_rgb, d_out = upload(stream, rgb), upload(stream, buf)
    d_rec = upload(stream, np.full(jl.RECORD_WORDS, 0x5A5A5A5A, np.int32))
    with torch.cuda.stream(stream):
        d_scratch = torch.full((n.value,), 0x3C, dtype=torch.uint8, device=dev)         # (whatever the scratch held before)
    a.rgb, a.scratch, a.scratch_bytes = d_rgb.data_ptr(), d_scratch.data_ptr(), n.value
    a.out, a.capacity, a.header_len, a.record = d_out.data_ptr(), capacity, jl.HEADER_LEN, d_rec.data_ptr()
    jl.check("rtj_encode", lib.rtj_encode(a, stream.cuda_stream))
    stream.synchronize()
    assert d_rgb.cpu().numpy().tobytes() == np.ascontiguousarray(rgb).tobytes()
    return d_out.cpu().numpy(), d_rec.cpu().numpy().view(np.uint32)

def same(name, out, rec, want, capacity):
    r = want["record"]
    over = int(r["total"] > capacity)
    assert rec.tolist() == [r["total"], r["raw"], r["stuffed"], r["intervals"], over, 0, 0, 0], (name, rec.tolist(), r)
    kept = min(r["total"], capacity)
    diff = np.flatnonzero(out[:kept] != np.frombuffer(want["file"], np.uint8)[:kept])
    assert diff.size == 0, (name, diff[:8], out[diff[:8]], [want["file"][i] for i in diff[:8]])
    assert (out[kept:] == SENTINEL).all(), (name, np.flatnonzero(out[kept:] != SENTINEL)[:8] + kept)
"""


def _child(body, *args, timeout=600):
    r = subprocess.run([sys.executable, "-c", _PRELUDE + body, *map(str, args)], capture_output=True, text=True, cwd=ROOT,
                       timeout=timeout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    return r.stdout


# ------------------------------------------------------------------------------------------- 1. the encoder, no scene

_CORPUS_CHILD = r"""
lib = jl.load()
stream = torch.cuda.Stream(device=dev)
seen = set()
for name, rgb, quality, interval in jnp.corpus():
    R, W = rgb.shape[:2]
    interval = (W + 7) // 8 if interval is None else interval
    want = jnp.encode(rgb, quality, interval)
    out, rec = device_encode(lib, stream, rgb, quality, interval)
    same(name, out, rec, want, len(out) - TAIL)
    seen.add((W, R, quality, interval))
    if name == "67x19 noise q100":
        stuffed, last_ff = jnp.stuffing_facts(want)
        assert stuffed > 0 and last_ff > 0
    if name == "67x19 single coefficient":
        assert any(0xF0 in jnp.symbols(b) for m in want["coef"] for b in m)
    if name == "67x19 flat grey":
        assert all(jnp.symbols(b) == [0x00] for m in want["coef"] for b in m)
    if name == "72x16 noise, interval 1":
        assert want["record"]["intervals"] == 18 and jnp.rst_markers(want["file"], jnp.HEADER_LEN) == [k % 8 for k in range(17)]
assert {(8, 8, 90, 1), (13, 21, 1, 2), (67, 19, 50, 3), (67, 19, 90, 1), (67, 19, 90, 9), (67, 19, 90, 28), (67, 19, 100, 1)} <= seen
print("ok")
"""

_LARGE_CHILD = r"""
lib = jl.load()
stream = torch.cuda.Stream(device=dev)
rgb = jnp.gradient(264, 264)
rgb[100:140, 60:200] = jnp.noise(40, 140, 7)
for interval in (1, 7):
    want = jnp.encode(rgb, 90, interval)
    assert len(want["mcu_bits"]) == 1089 and want["record"]["intervals"] == (1089 + interval - 1) // interval
    out, rec = device_encode(lib, stream, rgb, 90, interval)
    same(("264x264", interval), out, rec, want, len(out) - TAIL)
tables = (np.arange(128) % 31 + 1).astype(np.uint8)
want = jnp.encode(rgb, 0, 33, tables)
out, rec = device_encode(lib, stream, rgb, 0, 33, tables=tables)
same("264x264, the caller's tables", out, rec, want, len(out) - TAIL)
print("ok")
"""


def test_the_encoder_on_the_corpus(ndev):
    _child(_CORPUS_CHILD)


def test_more_than_a_chunk_of_mcus_and_of_intervals(ndev):
    _child(_LARGE_CHILD)


# ------------------------------------------------------------------------------------------- 2. overflow

_OVERFLOW_CHILD = r"""
lib = jl.load()
stream = torch.cuda.Stream(device=dev)
for name, rgb, quality, interval in ((n, f, q, i) for n, f, q, i in jnp.corpus() if n in ("67x19 noise q100", "72x16 noise, interval 1", "8x8 flat")):
    R, W = rgb.shape[:2]
    interval = (W + 7) // 8 if interval is None else interval
    want = jnp.encode(rgb, quality, interval)
    total = want["record"]["total"]
    for capacity in (total - 1, jl.HEADER_LEN + 1, total - 2, total):
        out, rec = device_encode(lib, stream, rgb, quality, interval, capacity=capacity)
        assert len(out) == capacity + TAIL and rec[4] == int(capacity < total) and rec[0] == total
        same((name, capacity), out, rec, want, capacity)
print("ok")
"""


def test_overflow(ndev):
    _child(_OVERFLOW_CHILD)


# ------------------------------------------------------------------------------------------- 3. the chain

_FILM_CHILD = r"""
from PIL import Image
W, H, DIV, SPP = 96, 54, 3, 8
sph, rq = scenes.config("c2")
strips = [rt.default_request(width=W, height=H, divisions=DIV, division_no=k, spp=SPP, max_bounces=rq.max_bounces, seed=rq.seed)
          for k in range(DIV)]

def refused(call, *a, **kw):
    try:
        call(*a, **kw)
    except ValueError:
        return True
    return False

with rt.Scene(0, rt.World(sph)) as scene:
    with rt.Film(scene, strips, integrator="nee", mode=rt.RT_NEE_MIS, moments=True) as film, rt.FilmDisplay(film) as display:
        film.render_pass(0, SPP)
        rgb = display.display(film.preview(("linear",))["linear"])["rgb"]
        film.sync()
        frame = rgb.cpu().numpy().copy()
        assert frame.shape == (H, W, 3) and frame.std() > 1
        with rt.FrameEncoder(film) as enc:
            assert enc.settings == ((H, W), 90, 16, 629 + H * W * 3)
            want = jnp.encode(frame, 90, 16)
            data = enc.encode(rgb)
            assert isinstance(data, bytes) and data == want["file"]
            im = Image.open(io.BytesIO(data))
            im.load()
            assert im.size == (W, H) and im.mode == "RGB"
            b = io.BytesIO()                                                         # the picture Pillow's own file of the frame gives
            Image.fromarray(frame).save(b, "JPEG", quality=90, subsampling=0, optimize=False, restart_marker_blocks=16)
            assert np.array_equal(np.asarray(im), np.asarray(Image.open(io.BytesIO(b.getvalue()))))
            assert enc.header == want["header"] == data[:629] and enc.bound == jnp.bound(W, H, 16)
            assert np.array_equal(np.array(enc.tables), jnp.quant_tables(90))
            out, record = enc.encode_device(rgb)                                     # nothing waits
            assert out.dtype == torch.uint8 and out.numel() == enc.capacity and record.shape == (8,)
            assert enc.record() == want["record"]
            assert rgb.cpu().numpy().tobytes() == frame.tobytes()
            assert refused(enc.encode, rgb[:, :-1]) and refused(enc.encode, rgb.float()) and refused(enc.encode, rgb.cpu())
            assert refused(enc.encode, frame) and refused(enc.encode, rgb.permute(1, 0, 2))
        # a capacity the file does not fit: one retry at the bound, which the encoder keeps
        with rt.FrameEncoder(film, quality=100, interval=5, capacity=1000) as small:
            want = jnp.encode(frame, 100, 5)
            assert want["record"]["total"] > 1000
            assert small.encode(rgb) == want["file"] and small.capacity == small.bound
            assert small.encode(rgb) == want["file"]
        # a frame of another size on the film's device and stream
        other = jnp.noise(19, 67, 11)
        with rt.FrameEncoder(film, shape=(19, 67), quality=50, interval=64) as enc:
            with torch.cuda.stream(film.stream):
                d = torch.from_numpy(other).to(dev)
            assert enc.encode(d) == jnp.encode(other, 50, 64)["file"]
        closed = rt.FrameEncoder(film)
        closed.close()
        closed.close()
        assert refused(closed.encode, rgb)
print("ok")
"""


def test_a_film_through_its_display_and_its_encoder(ndev):
    _child(_FILM_CHILD)
