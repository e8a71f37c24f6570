"""ANSI streams with frames in flight (ycge_render_frame_async_ansi) on the GPU.

1: k_ansi_deliver alone through its hook (ycge_test_ansi_deliver): exactly `length` bytes of random source bytes arrive, a canary from
   `length` on stays, the record holds what the device words held; the refusal of a stream above the capacity and of a misaligned buffer.
2: frames.  The yardstick everywhere is the synchronous export of the same form on a twin context (test_gpu_ansi_stream.twins), which the
   other ANSI test files hold byte for byte to the restatements - so every comparison here is for equality: stream, length, info, SDR bits.
"""
import ctypes as C

import numpy as np
import pytest

import parity_util as pu
import test_gpu_ansi_stream as S
from yetanotherconsolegameengine_amd import abi, scenes
from yetanotherconsolegameengine_amd.renderer import ConsoleLayer, RaytraceRenderer
from yetanotherconsolegameengine_amd.scene import flatten

pytestmark = pytest.mark.gpu
CANARY = S.CANARY
U8P = C.POINTER(C.c_uint8)
FULL_INFO = dict(keyframe=1, changed=0, emitted=0, runs=0)


# ------------------------------------------------------------------------------------------------------------- 1: the kernel alone
@pytest.fixture(scope="module")
def enc(product_lib):
    g = RaytraceRenderer(None, 16, 8, 45.0, 1)
    yield g
    g.close()


def deliver_hook(g):
    fn = g.L.ycge_test_ansi_deliver
    fn.restype, fn.argtypes = abi.ANSI_FLIGHT_HOOK_PROTOTYPES["ycge_test_ansi_deliver"]
    return fn


def record_of(rec):
    r = abi.AnsiAsyncResult.from_buffer_copy(rec.tobytes())
    return int(r.length), tuple(int(v) for v in r.info), int(r.status), int(r.reserved)


def deliver(g, src, length, capacity, keyframe=0, counts=(5, 7, 3), groups=0, dst_offset=0, rec_offset=0):
    """ycge_test_ansi_deliver into a canary-filled page-locked destination 64 bytes longer than `capacity` -> (rc, destination, record)"""
    out = g._page_locked_zeros((capacity + 64 + 16,), np.uint8)[0]
    rec = g._page_locked_zeros((C.sizeof(abi.AnsiAsyncResult) + 8,), np.uint8)[0]
    assert out.ctypes.data % 16 == 0 and rec.ctypes.data % 8 == 0
    out[...] = CANARY
    rec[...] = 0xEE
    src = np.ascontiguousarray(src, np.uint8)
    rc = deliver_hook(g)(g.ctx, src.ctypes.data if src.size else None, src.size, length, capacity, keyframe, (C.c_uint32 * 3)(*counts), groups,
                         out.ctypes.data + dst_offset, rec.ctypes.data + rec_offset)
    return rc, out[dst_offset:dst_offset + capacity + 64], rec[rec_offset:rec_offset + C.sizeof(abi.AnsiAsyncResult)]


def check_delivery(g, length, capacity, groups, seed):
    src = np.random.default_rng(seed).integers(0, 256, length, dtype=np.uint8)
    rc, out, rec = deliver(g, src, length, capacity, 0, (length % 11, 7, 3), groups)
    assert rc == abi.YCGE_OK, g.L.ycge_last_error(g.ctx)
    assert np.array_equal(out[:length], src), (length, groups, int(np.argmax(out[:length] != src)))
    assert (out[length:] == CANARY).all(), (length, groups, "a byte at or past the length was written")
    assert record_of(rec) == (length, (0, length % 11, 7, 3), 0, 0), (length, record_of(rec))


@pytest.mark.parametrize("length", [0, 1, 15, 16, 17, 4095, 4096, 4097])
def test_deliver_lengths_with_the_products_grid(enc, length):
    check_delivery(enc, length, length + 101, 0, length)
    check_delivery(enc, length, length, 0, length + 1)              # (the capacity reached exactly)


@pytest.mark.parametrize("length", [8191, 8192, 8193, 16385])
def test_deliver_across_the_grid_stride_wrap(enc, length):
    """two workgroups: one grid-stride pass is 2 x 256 x 16 = 8192 bytes"""
    check_delivery(enc, length, length + 37, 2, length)


def test_deliver_a_full_streams_size(enc):
    check_delivery(enc, 3_200_003, 3_200_003 + 4096, 0, 32)


def test_deliver_keyframe_record(enc):
    """a full stream's scan writes the length alone: the record's counts are 0 whatever the other words hold, as deliver() has them"""
    src = np.arange(100, dtype=np.uint8)
    rc, out, rec = deliver(enc, src, 100, 128, 1, (9, 9, 9))
    assert rc == abi.YCGE_OK
    assert np.array_equal(out[:100], src) and (out[100:] == CANARY).all()
    assert record_of(rec) == (100, (1, 0, 0, 0), 0, 0)


def test_deliver_above_the_capacity_copies_nothing_and_fails_the_join_once(enc):
    cap = 1000
    src = np.random.default_rng(3).integers(0, 256, cap + 1, dtype=np.uint8)
    rc, out, rec = deliver(enc, src, cap + 1, cap)
    assert rc == abi.YCGE_OK
    assert (out == CANARY).all(), "nothing may be written"
    length, info, status, _ = record_of(rec)
    assert (length, status) == (cap + 1, 1)
    assert enc.L.ycge_wait(enc.ctx) == abi.YCGE_ERR_DEVICE
    assert b"capacity" in enc.L.ycge_last_error(enc.ctx)
    assert enc.L.ycge_wait(enc.ctx) == abi.YCGE_OK
    check_delivery(enc, 777, 1000, 0, 4)


def test_deliver_refuses_misaligned_and_pageable_buffers(enc):
    src = np.arange(64, dtype=np.uint8)
    rc, out, rec = deliver(enc, src, 64, 64, dst_offset=8)
    assert rc == abi.YCGE_ERR_INVALID_ARG and b"16-byte aligned" in enc.L.ycge_last_error(enc.ctx)
    assert (out == CANARY).all() and (rec == 0xEE).all()
    rc, out, rec = deliver(enc, src, 64, 64, rec_offset=4)
    assert rc == abi.YCGE_ERR_INVALID_ARG and b"8-byte aligned" in enc.L.ycge_last_error(enc.ctx)
    assert (out == CANARY).all() and (rec == 0xEE).all()
    pageable, locked_rec = np.full(256, CANARY, np.uint8), enc._page_locked_zeros((32,), np.uint8)[0]
    at = pageable.ctypes.data + (-pageable.ctypes.data) % 16
    rc = deliver_hook(enc)(enc.ctx, src.ctypes.data, 64, 64, 64, 0, (C.c_uint32 * 3)(), 0, at, locked_rec.ctypes.data)
    assert rc == abi.YCGE_ERR_INVALID_ARG and b"page-locked" in enc.L.ycge_last_error(enc.ctx)
    assert (pageable == CANARY).all()
    assert enc.L.ycge_wait(enc.ctx) == abi.YCGE_OK


# ------------------------------------------------------------------------------------------------------------- 2: frames
FORMS = [(False, False), (False, True), (True, False), (True, True)]          # (rgb, delta)
FORM_IDS = ["ansi", "ansi_delta", "ansi_rgb", "ansi_rgb_delta"]
CASES = [c for c in S.FRAME_CASES if c in ((1, 80, 45, 1), (2, 160, 45, 1), (5, 160, 45, 1))]
SEQ = [0, 0, 0, 1, 1, 1]


def sync_frame(g, rgb, delta, cw, ch, merge_gap=3, tolerance=0, keyframe=False, **base):
    """the synchronous export of the form -> (bytes, info, SDR); a full stream's info is what the in-flight record holds for one"""
    if delta and rgb:
        return g.TryFlipAndBlitAnsiRgbDelta(cw, ch, merge_gap=merge_gap, tolerance=tolerance, keyframe=keyframe, sdr=True, **base)
    if delta:
        return g.TryFlipAndBlitAnsiDelta(cw, ch, merge_gap=merge_gap, keyframe=keyframe, sdr=True, **base)
    stream, sdr = (g.TryFlipAndBlitAnsiRgb if rgb else g.TryFlipAndBlitAnsi)(cw, ch, sdr=True, **base)
    return stream, dict(FULL_INFO), sdr


def queue_frame(g, slot, rgb, delta, cw, ch, **kw):
    """RenderAsyncAnsi with the slot's buffer full of canaries (from its second use on: the first finds it zeroed)"""
    ring = g.__dict__.get("_ansi_ring", {})
    if slot in ring:
        ring[slot]["stream"][...] = CANARY
        ring[slot]["fill"] = CANARY
    g.RenderAsyncAnsi(slot, cw, ch, rgb=rgb, delta=delta, sdr=True, **kw)
    g._ansi_ring[slot].setdefault("fill", 0)


def result(g, slot):
    stream, info, sdr = g.AsyncAnsiResult(slot)
    entry = g._ansi_ring[slot]
    assert (entry["stream"][len(stream):] == entry["fill"]).all(), "bytes at or past the stream's length were written"
    return stream, info, sdr.copy()


def assert_frame(got, want, what):
    S.assert_stream(got[0], want[0], what)
    assert got[1] == want[1], (what, got[1], want[1])
    assert pu.bits_equal(got[2], want[2]), what


@pytest.mark.parametrize("ring", [6, 2], ids=["six-slots", "ring-of-two"])
@pytest.mark.parametrize("rgb,delta", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("n,w,h,ss", CASES, ids=[f"c{c[0]}" for c in CASES])
def test_queued_frames_equal_the_synchronous_twin(product_lib, n, w, h, ss, rgb, delta, ring):
    a, b, pose = S.twins(n, w, h, ss)
    try:
        cw, ch = w + 1, h
        kw = dict(merge_gap=2, tolerance=1 if rgb else 0) if delta else {}
        want = []
        for k in SEQ:
            S.move((a,), pose, k)
            want.append(sync_frame(a, rgb, delta, cw, ch, **kw))
        got, pending = [], []
        for i, k in enumerate(SEQ):
            S.move((b,), pose, k)
            queue_frame(b, i % ring, rgb, delta, cw, ch, **kw)
            pending.append(i % ring)
            if len(pending) == min(ring, len(SEQ)) or i == len(SEQ) - 1:
                b.Wait()
                got += [result(b, s) for s in pending]
                pending = []
        fi = b.flight_info()
        assert fi["post_pair"] == 1 if n in (1, 2) else fi["stage_pipeline"] == 1, fi          # (side by side on two streams / one behind the other)
        for i in range(len(SEQ)):
            assert_frame(got[i], want[i], f"config {n} {FORM_IDS[FORMS.index((rgb, delta))]} frame {i}")
        if delta:
            assert [g[1]["keyframe"] for g in got] == [1, 0, 0, 0, 0, 0]
        assert pu.bits_equal(a.read(abi.BUF_TAA_HISTORY), b.read(abi.BUF_TAA_HISTORY))
    finally:
        a.close(); b.close()


def console_layers(k):
    """a console-sized text layer below the raytrace framebuffer (mostly transparent) and a 10 x 3 one above it, for an 81 x 45 console"""
    rows = [" " * 81 for _ in range(45)]
    rows[0] = ("frame_%d_" % k).ljust(81, "=")
    rows[44] = ("hud %03d" % (7 * k)).rjust(81)
    below = ConsoleLayer(rows, fg=(0.9, 0.9, 0.2), bg=(0.0, 0.0, 0.3))
    above = ConsoleLayer(["+--------+", ("|menu__%d |" % k), "+--------+"], fg=(1.0, 1.0, 1.0), bg=(0.4, 0.0, 0.0), x=5 + k, y=4)
    return [below, above]


@pytest.mark.parametrize("rgb", [False, True], ids=["256", "rgb"])
def test_layers_in_force_with_an_edit_between_queued_frames(product_lib, rgb):
    a, b, pose = S.twins(1, 80, 45, 1)
    try:
        kw = dict(merge_gap=3, tolerance=0)
        for g in (a, b):
            g.SetConsoleLayers(console_layers(0), 1)
        want = []
        for k in range(6):
            S.move((a, b), pose, k // 2)
            if k == 3:
                a.SetConsoleLayers(console_layers(1), 1)
                b.SetConsoleLayers(console_layers(1), 1)          # (joins the three frames in flight)
            want.append(sync_frame(a, rgb, True, 81, 45, **kw))
            queue_frame(b, k, rgb, True, 81, 45, **kw)
        b.Wait()
        for k in range(6):
            got = result(b, k)
            assert_frame(got, want[k], f"layers rgb={rgb} frame {k}")
            assert got[1]["keyframe"] == (1 if k == 0 else 0)
        assert b"menu__0" in want[0][0] and b"menu__1" in want[3][0]
    finally:
        a.close(); b.close()


def test_delta_state_rules_hold_for_queued_calls(product_lib):
    a, b, pose = S.twins(1, 80, 45, 1)
    try:
        cw, ch = 81, 45
        step = [0]

        def both(rgb, delta, queued, slot=0, **kw):
            """the next frame on both contexts: synchronously on a; on b queued into `slot` (and waited for) or synchronously"""
            S.move((a, b), pose, step[0] // 2)
            step[0] += 1
            want = sync_frame(a, rgb, delta, cw, ch, **kw)
            if not queued:
                got = sync_frame(b, rgb, delta, cw, ch, **kw)
            else:
                queue_frame(b, slot, rgb, delta, cw, ch, **kw)
                return want, None
            assert_frame(got, want, f"step {step[0]}")
            return want, got

        def collect(wants):
            b.Wait()
            out = []
            for slot, want in wants:
                out.append(result(b, slot))
                assert_frame(out[-1], want, f"slot {slot}")
            return out

        # a synchronous _ansi between queued deltas: the next queued delta is a keyframe
        w0, _ = both(False, True, True, 0)
        w1, _ = both(False, True, True, 1)
        both(False, False, False)
        w2, _ = both(False, True, True, 2)
        got = collect([(0, w0), (1, w1), (2, w2)])
        assert [g[1]["keyframe"] for g in got] == [1, 0, 1]
        # a synchronous _ansi_delta behind two queued deltas is a delta, the twin's third
        w0, _ = both(False, True, True, 0)
        w1, _ = both(False, True, True, 1)
        want, got3 = both(False, True, False)
        assert got3[1]["keyframe"] == 0 and want[1]["keyframe"] == 0
        collect([(0, w0), (1, w1)])
        # a queued 24-bit delta behind a queued 256-colour delta is a keyframe, and so is the 256-colour one behind it (twice: the second
        # time every buffer of both forms exists, so nothing joins the frames in flight between the four)
        for _ in range(2):
            w0, _ = both(False, True, True, 0)
            w1, _ = both(True, True, True, 11)
            w2, _ = both(True, True, True, 12)
            w3, _ = both(False, True, True, 3)
            got = collect([(0, w0), (11, w1), (12, w2), (3, w3)])
            assert [g[1]["keyframe"] for g in got] == [0, 1, 0, 1]
        # Resize: a keyframe
        w0, _ = both(False, True, True, 0)
        a.Resize(96, 30, 1); b.Resize(96, 30, 1)
        cw, ch = 97, 30
        w1, _ = both(False, True, True, 1)
        w2, _ = both(False, True, True, 2)
        b.Wait()
        got = [result(b, 1), result(b, 2)]
        assert_frame(got[0], w1, "after Resize"); assert_frame(got[1], w2, "after Resize, the second")
        assert [g[1]["keyframe"] for g in got] == [1, 0]
        assert pu.bits_equal(a.read(abi.BUF_TAA_HISTORY), b.read(abi.BUF_TAA_HISTORY))
    finally:
        a.close(); b.close()


def test_buffers_grow_under_queued_frames(product_lib):
    """queued calls whose buffers must grow while frames are in flight - each in a slot of its own, no Wait between them: every frame equals
    the synchronous twin's, whichever buffer its call had to make"""
    a, b, pose = S.twins(1, 80, 45, 1)
    try:
        steps = [(False, False, 41, 23),          # a 256-colour full stream
                 (False, True, 41, 23),           # its delta form: a keyframe, the held pairs
                 (False, True, 81, 45),           # the stream and the tiles grow; another geometry: a keyframe
                 (True, True, 81, 45),            # 24-bit: the triples' palette, a held plane of 8 bytes a cell
                 (True, True, 81, 45),            # a real delta
                 (True, True, 81, 45),            # (layers set in front) the composite's planes and the third colour plane
                 (False, True, 161, 46)]          # a console larger than the framebuffer: the composite grows
        want = []
        for k, (rgb, delta, cw, ch) in enumerate(steps):
            S.move((a, b), pose, k // 2)
            if k == 5:
                for g in (a, b):
                    g.SetConsoleLayers(console_layers(0), 1)
            kw = dict(merge_gap=3, tolerance=0) if delta else {}
            want.append(sync_frame(a, rgb, delta, cw, ch, **kw))
            queue_frame(b, k, rgb, delta, cw, ch, **kw)
        b.Wait()
        got = [result(b, k) for k in range(len(steps))]
        for k in range(len(steps)):
            assert_frame(got[k], want[k], f"growing buffers, frame {k}")
        assert [g[1]["keyframe"] for g in got] == [1, 1, 1, 1, 0, 1, 1]
        assert b"menu__0" in want[5][0] and b"menu__0" in want[6][0]
        assert pu.bits_equal(a.read(abi.BUF_TAA_HISTORY), b.read(abi.BUF_TAA_HISTORY))
    finally:
        a.close(); b.close()


def test_interleaved_with_the_other_frames_in_flight(product_lib):
    """RenderAsync(sdr_slot) and RenderAsyncChexels frames between RenderAsyncAnsi frames on one context: every output equals the twin's"""
    a, b, pose = S.twins(2, 160, 45, 1)
    try:
        cw, ch = 161, 45
        plan = [("ansi", False, True), ("sdr",), ("ansi", False, True), ("chexels",), ("ansi", True, False), ("ansi", True, True), ("sdr",), ("ansi", True, True),
                ("chexels",), ("ansi", False, True)]
        want, queued = [], []
        for k, stp in enumerate(plan):
            S.move((a, b), pose, k // 3)
            if stp[0] == "ansi":
                want.append(sync_frame(a, stp[1], stp[2], cw, ch))
                queue_frame(b, k, stp[1], stp[2], cw, ch)
                queued.append(None)
            elif stp[0] == "sdr":
                want.append(a.TryFlipAndBlit(want_sdr=True))
                queued.append(b.RenderAsync(sdr_slot=k))
            else:
                want.append(a.TryFlipAndBlitChexels(color16=True, ansi=True, rgba=True, sdr=True))
                queued.append(b.RenderAsyncChexels(k, color16=True, ansi=True, rgba=True, sdr=True))
        b.Wait()
        for k, stp in enumerate(plan):
            if stp[0] == "ansi":
                assert_frame(result(b, k), want[k], f"interleaved step {k}")
            elif stp[0] == "sdr":
                assert pu.bits_equal(queued[k], want[k]), k
            else:
                for name in ("sdr", "color16", "ansi", "rgba"):
                    assert pu.bits_equal(queued[k][name], want[k][name]) if name == "sdr" else np.array_equal(queued[k][name], want[k][name]), (k, name)
        assert pu.bits_equal(a.read(abi.BUF_TAA_HISTORY), b.read(abi.BUF_TAA_HISTORY))
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------- 3: refusals
def raw_call(g, req, out, cap, rec, sdr=None):
    ptr = lambda x: (x if isinstance(x, int) else x.ctypes.data) if x is not None else None
    return g.L.ycge_render_frame_async_ansi(g.ctx, C.byref(req) if req is not None else None, C.cast(ptr(out), U8P) if out is not None else None, cap, ptr(rec),
                                            C.cast(ptr(sdr), C.POINTER(C.c_float)) if sdr is not None else None)


def request(cw=81, ch=45, vp=(0, 0), fg=7, bg=0, clear=0, rgb=0, delta=0, gap=0, tol=0, key=0):
    return abi.AnsiAsync(cw, ch, vp[0], vp[1], fg, bg, clear, rgb, delta, gap, tol, key)


def test_refusals_name_the_argument_and_leave_the_delta_state(product_lib):
    a, b, pose = S.twins(1, 80, 45, 1)
    L = b.L
    try:
        cw, ch = 81, 45
        w0 = sync_frame(a, False, True, cw, ch)
        w1 = sync_frame(a, False, True, cw, ch)
        queue_frame(b, 0, False, True, cw, ch)
        queue_frame(b, 1, False, True, cw, ch)
        cap = RaytraceRenderer.ansi_stream_bound(cw, ch, L)
        cap_rgb = RaytraceRenderer.ansi_rgb_stream_bound(cw, ch, L)
        out = b._page_locked_zeros((cap_rgb + 64,), np.uint8)[0]
        rec = b._page_locked_zeros((40,), np.uint8)[0]
        sdr = b._page_locked_zeros((45, 80, 2, 3))[0]
        heap_out, heap_rec, heap_sdr = np.zeros(cap + 64, np.uint8), np.zeros(40, np.uint8), np.zeros((45, 80, 2, 3), np.float32)
        heap_at = heap_out.ctypes.data + (-heap_out.ctypes.data) % 16
        heap_rec_at = heap_rec.ctypes.data + (-heap_rec.ctypes.data) % 8
        assert L.ycge_render_frame_async_ansi(None, C.byref(request()), out.ctypes.data_as(U8P), cap, rec.ctypes.data, None) == abi.YCGE_ERR_INVALID_ARG
        refusals = [
            ((None, out, cap, rec), [b"req"]),
            ((request(), None, cap, rec), [b"out_stream", b"NULL"]),
            ((request(), out, cap, None), [b"out_result", b"NULL"]),
            ((request(), heap_at, cap, rec), [b"out_stream", b"page-locked"]),
            ((request(), out, out.size + (1 << 20), rec), [b"out_stream", b"page-locked", b"%d" % (out.size + (1 << 20))]),
            ((request(), out.ctypes.data + 8, cap, rec), [b"out_stream", b"16-byte aligned"]),
            ((request(), out, cap, heap_rec_at), [b"out_result", b"page-locked"]),
            ((request(), out, cap, rec.ctypes.data + 4), [b"out_result", b"8-byte aligned"]),
            ((request(), out, cap, rec, heap_sdr), [b"out_top_bottom_sdr", b"page-locked"]),
            ((request(), out, cap - 1, rec), [b"capacity %d" % (cap - 1), b"bound %d" % cap]),
            ((request(rgb=1), out, cap_rgb - 1, rec), [b"capacity %d" % (cap_rgb - 1), b"bound %d" % cap_rgb]),
            ((request(delta=1, gap=9), out, cap, rec), [b"merge_gap 9"]),
            ((request(delta=1, gap=-1), out, cap, rec), [b"merge_gap -1"]),
            ((request(rgb=1, delta=1, tol=256), out, cap_rgb, rec), [b"tolerance 256"]),
            ((request(rgb=1, delta=1, tol=-1), out, cap_rgb, rec), [b"tolerance -1"]),
            ((request(delta=1, tol=3), out, cap, rec), [b"tolerance 3", b"rgb"]),
            ((request(gap=2), out, cap, rec), [b"merge_gap 2", b"full stream"]),
            ((request(rgb=1, tol=5), out, cap_rgb, rec), [b"tolerance 5", b"full stream"]),
            ((request(key=1), out, cap, rec), [b"keyframe 1", b"full stream"]),
            ((request(cw=0), out, cap, rec), [b"positive"]),
            ((request(fg=16), out, cap, rec), [b"0..15"]),
            ((request(cw=100000, ch=2000), out, cap, rec), [b"2^32"]),
        ]
        for args, words in refusals:
            rc = raw_call(b, *args)
            msg = L.ycge_last_error(b.ctx)
            assert rc == abi.YCGE_ERR_INVALID_ARG, (words, rc, msg)
            for wd in words:
                assert wd in msg, (words, msg)
        # the next queued delta is what it would have been: the twin's third, a delta
        w2 = sync_frame(a, False, True, cw, ch)
        queue_frame(b, 2, False, True, cw, ch)
        b.Wait()
        for slot, want in enumerate((w0, w1, w2)):
            got = result(b, slot)
            assert_frame(got, want, f"slot {slot}")
            assert got[1]["keyframe"] == (1 if slot == 0 else 0)
        assert not out.any() and not rec.any() and not sdr.any() and not heap_out.any() and not heap_rec.any() and not heap_sdr.any()
    finally:
        a.close(); b.close()


def test_contexts_the_frames_in_flight_refuse(product_lib):
    sc, w, h, ss, pose = scenes.config_scene(1)
    flat = flatten(sc)
    cfg = abi.default_config()
    cfg.multi_device_exchange = abi.EXCHANGE_RCCL
    cases = [(dict(capture_debug=True), b"debug captures"), (dict(count_work=True), b"per-frame counters"), (dict(devices=[0, 0]), b"single-device"),
             (dict(cfg=cfg, devices=[0], slab_albedo=False), b"lean slabs")]
    for kw, word in cases:
        g = RaytraceRenderer(flat, 80, 45, pose["fov"], 1, **kw)
        try:
            cap = RaytraceRenderer.ansi_stream_bound(81, 45, g.L)
            out, rec = g._page_locked_zeros((cap,), np.uint8)[0], g._page_locked_zeros((32,), np.uint8)[0]
            rc = raw_call(g, request(delta=1, gap=3), out, cap, rec)
            assert rc == abi.YCGE_ERR_INVALID_ARG and word in g.L.ycge_last_error(g.ctx), (kw, rc, g.L.ycge_last_error(g.ctx))
            assert g.L.ycge_wait(g.ctx) == abi.YCGE_OK
            assert not out.any() and not rec.any()
            stream, info = g.TryFlipAndBlitAnsiDelta(81, 45)[:2] if "slab_albedo" not in kw else (b"", FULL_INFO)
            assert info["keyframe"] == 1
        finally:
            g.close()
