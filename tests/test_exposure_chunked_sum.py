"""CPU check of the ALGORITHM behind k_exposure_sum (csrc/ycge_post.hip): the reference's serial binary32 sum
(ToneMapper.cs:63-77) evaluated chunk by chunk as integer arithmetic inside one binade, with the serial loop as the fallback.
This is a line-for-line Python twin of the kernel's three phases, its groups of 16 chunks and its batches of 1024 included; the
kernels themselves are held to the serial loop's logSum bits by tests/test_gpu_post_probe.py (-m gpu) on the same term families."""
import math
import struct

import numpy as np
import pytest


def f2u(f):
    return struct.unpack("<I", struct.pack("<f", f))[0]


def u2f(u):
    return struct.unpack("<f", struct.pack("<I", u))[0]


def chunked_sum(terms, CH=512, BATCH=1024, drop_tie_rule=False, drop_batch_parity=False):
    n = len(terms)
    nch = (n + CH - 1) // CH
    csum = [float(np.sum(terms[c * CH:(c + 1) * CH].astype(np.float64))) for c in range(nch)]       # phase A
    chunks, pre = [], 0.0
    for c in range(nch):                                                                            # phase B
        s0 = pre
        pre += csum[c]
        neg = 1 if s0 < 0 else 0
        e = -1000                               # (a NaN prefix compares false: -1000; an infinite one has the exponent field 2047)
        if abs(s0) >= 1e-30:
            e = 1024 if math.isinf(s0) else math.frexp(abs(s0))[1] - 1
        C = dict(e=e, neg=neg, d=[0, 0], lo=[0, 0], hi=[0, 0])
        if not np.any(terms[c * CH:(c + 1) * CH]):
            C["e"] = -2000                      # nothing but + 0.0f: leaves any sum as it is
        elif -12 <= e < 100:
            inv_u = (2.0 ** (23 - e)) * (-1.0 if neg else 1.0)
            d, lo, hi, p = [0, 0], [0, 0], [0, 0], [0, 1]
            for t in terms[c * CH:(c + 1) * CH]:
                x = float(t) * inv_u
                if not (-1.0e12 < x < 1.0e12):          # absurd term (inf / nan / 1e30): this chunk never takes the fast path
                    lo = [-(1 << 62), -(1 << 62)]
                    continue
                fx = math.floor(x)
                fr = x - fx
                ifx = int(fx)
                for k in (0, 1):
                    inc = ((p[k] + ifx) & 1) if fr == 0.5 and not drop_tie_rule else (1 if fr > 0.5 else 0)
                    d[k] += ifx + inc
                    p[k] = (p[k] + ifx + inc) & 1
                    lo[k] = min(lo[k], d[k])
                    hi[k] = max(hi[k], d[k])
            C.update(d=d, lo=lo, hi=hi)
        else:
            C["e"] = -1000                      # below 2^-12 (the sum is still tiny) or absurdly large: serial
        chunks.append(C)
    s, n_serial = np.float32(0), 0
    for batch in range(0, nch, BATCH):                                                              # phase C, a batch of records at a time
        batch_end = min(batch + BATCH, nch)
        # groups of 16 chunks of this batch composed into one map each (the kernel's two-level walk); a ragged last group is not composed
        groups = []
        for k0 in range(0, BATCH, 16):
            ok = batch + k0 + 16 <= batch_end
            G = dict(ok=ok, d=[0, 0], lo=[0, 0], hi=[0, 0])
            if ok:
                g0 = batch + k0
                G["ok"] = all(chunks[g0 + j]["e"] == -2000 or (chunks[g0 + j]["e"] == chunks[g0]["e"] and chunks[g0 + j]["neg"] == chunks[g0]["neg"] and chunks[g0]["e"] > -1000)
                              for j in range(16))
                for pin in (0, 1):
                    D, L, H, P = 0, 0, 0, pin
                    for j in range(16):
                        Ck = chunks[g0 + j]
                        if Ck["e"] == -2000:
                            continue
                        L = min(L, D + Ck["lo"][P]); H = max(H, D + Ck["hi"][P])
                        dk = Ck["d"][P]
                        D += dk
                        P = (P + dk) & 1
                    G["d"][pin], G["lo"][pin], G["hi"][pin] = D, L, H
            groups.append(G)
        c = batch
        while c < batch_end:
            C = chunks[c]
            k = c - batch
            bits = f2u(float(s))
            ex = (bits >> 23) & 0xff
            m = (bits & 0x7fffff) | 0x800000
            p = m & 1
            if drop_batch_parity and batch > 0 and k == 0:
                p = 0                               # (a deliberately wrong twin: the sum's parity is not carried into the next batch)
            if C["e"] == -2000:
                c += 1
                continue
            if k % 16 == 0 and groups[k // 16]["ok"]:
                G = groups[k // 16]
                if ex != 0 and ex - 127 == C["e"] and (bits >> 31) == C["neg"] and m + G["lo"][p] > (1 << 23) and m + G["hi"][p] < (1 << 24):
                    s = np.float32(u2f((bits & 0xff800000) | ((m + G["d"][p]) & 0x7fffff)))
                    c += 16
                    continue
            fast = ex != 0 and ex - 127 == C["e"] and (bits >> 31) == C["neg"] and m + C["lo"][p] > (1 << 23) and m + C["hi"][p] < (1 << 24)
            if fast:
                s = np.float32(u2f((bits & 0xff800000) | ((m + C["d"][p]) & 0x7fffff)))
            else:
                with np.errstate(all="ignore"):
                    for t in terms[c * CH:(c + 1) * CH]:
                        s = np.float32(s + t)
                n_serial += 1
            c += 1
    return s, n_serial, nch


@pytest.mark.parametrize("trial", range(6))
def test_chunked_evaluation_equals_the_serial_binary32_sum(trial):
    rng = np.random.default_rng(5 + trial)
    n = 30000 + trial * 3777
    lum = rng.random(n).astype(np.float32) ** np.float32(2 + trial)
    terms = np.log(np.float32(1e-6) + lum).astype(np.float32)
    if trial % 2:
        terms[rng.random(n) < 0.3] = np.float32(0)                      # skipped samples contribute +0
        terms[:7000] = np.float32(0); terms[20000:23000] = np.float32(0)  # whole chunks of sky, at the start and inside
    if trial == 4:
        terms = np.abs(terms) * np.float32(0.01)                        # a positive, slowly growing sum
    if trial == 5:
        terms = (terms + np.float32(5.0)).astype(np.float32)            # mixed signs
    idx = rng.integers(0, n, 1500)                                      # exact ties: dyadic terms
    terms[idx] = (rng.integers(-64, 64, 1500) / np.float32(32.0)).astype(np.float32)
    ref = np.float32(0)
    for t in terms:
        ref = np.float32(ref + t)
    got, n_serial, nch = chunked_sum(terms)
    assert f2u(float(ref)) == f2u(float(got))
    assert n_serial < nch // 3              # the fast path carries the bulk


def _same(a, b):
    return (np.isnan(a) and np.isnan(b)) or f2u(float(a)) == f2u(float(b))


@pytest.mark.parametrize("family", __import__("post_probe_inputs").EXPOSURE_FAMILIES)
def test_twin_on_the_term_families_of_the_device_tests(family):
    """The families tests/test_gpu_post_probe.py feeds the kernels, at the lengths around one chunk, one group of 16 and (for a few) one
    batch of 1024 chunks: the twin's logSum is the serial loop's, NaN for NaN."""
    import post_probe_inputs as ppi
    lengths = [1, 3, 511, 512, 513, 1023, 8191, 8192, 8193]
    if family in ("dark", "dyadic_odd", "nan_last"): lengths.append(524289)          # (a second batch; pure Python: kept to three families)
    for n in lengths:
        terms = ppi.exposure_terms(family, n, seed=1)
        ref = ppi.serial_sum_f32(terms)
        got, n_serial, nch = chunked_sum(terms)
        assert _same(ref, got), (family, n, float(ref), float(got))
        if n >= 131072 and family in ppi.EXPOSURE_TAME:
            assert n_serial < nch // 3, (family, n, n_serial, nch)


def test_cumulative_sum_is_the_serial_loop():
    import post_probe_inputs as ppi
    terms = ppi.exposure_terms("dark", 5000, seed=2)
    ref = np.float32(0)
    for t in terms:
        ref = np.float32(ref + t)
    assert f2u(float(ref)) == f2u(float(ppi.serial_sum_f32(terms)))


def test_the_twin_notices_a_dropped_tie_rule_and_a_dropped_batch_parity():
    """what the families are for: without round-half-to-even on exact ties, or with the parity not carried across a batch, the dyadic
    families no longer give the serial sum"""
    import post_probe_inputs as ppi
    terms = ppi.exposure_terms("dyadic_odd", 8193, seed=1)
    ref = ppi.serial_sum_f32(terms)
    assert _same(ref, chunked_sum(terms)[0]) and not _same(ref, chunked_sum(terms, drop_tie_rule=True)[0])
    terms = ppi.exposure_terms("dyadic_odd", 40 * 512 + 5, seed=1)
    ref = ppi.serial_sum_f32(terms)
    bad = [not _same(ref, chunked_sum(ppi.exposure_terms(f, 40 * 512 + 5, seed=sd), BATCH=16, drop_batch_parity=True)[0]) and
           _same(ppi.serial_sum_f32(ppi.exposure_terms(f, 40 * 512 + 5, seed=sd)), chunked_sum(ppi.exposure_terms(f, 40 * 512 + 5, seed=sd), BATCH=16)[0])
           for f in ("dyadic_even", "dyadic_odd") for sd in (1, 2, 3)]
    assert any(bad), bad
