"""CPU: the padding poisoner of tests/_padding.py and what a comparison on
poisoned padding can see.

tests/test_gpu_nonfinite_padding.py overwrites the padding rows of the exact
corpora with NaN / Inf encodings and requires every path to return the clean
reference's bits.  Here, without a GPU:
  (a) the poisoner changes every padding row and nothing else, on numpy arrays
      and torch tensors alike, and the decoded padding is non-finite where its
      mode says so;
  (b) the exact reference (tests/_exact.py) is a function of the scoring rows
      only: a brute-force float64 scorer that SELECTS the scoring rows returns
      the reference's bits on the poisoned encodings, so no expected score
      moves;
  (c) the comparison would notice a leak: the same scorer masking the way the
      kernels do (the padding rows of a partly filled 16-row tile start at
      -inf, the products are added on top) and folding with np.maximum, which
      keeps a NaN, differs from the reference on a doc of every doclens % 16
      != 0 class in both modes, while folding with np.fmax, which drops it,
      equals the reference;
  (d) the walks replayed on poisoned pools (tests/_walk_seeds.PADDING_SEEDS)
      call every entry point on every (kind, ld) and put every value of every
      handle option in force, and no shorter prefix does.
"""
import functools

import numpy as np
import pytest
import torch

import _exact as ex
import _padding as pd
import _walk as wk
import _walk_seeds as ws
from oracle import oracle as orc

LD, N, B = 128, 176, 33          # the corpus of tests/test_exact_corpus.py
NQ = 6                           # queries scored by the brute-force scorer


@functools.lru_cache(maxsize=None)
def corpus(kind):
    return ex.ExactCorpus(kind, LD, N, B, seed=5)


@functools.lru_cache(maxsize=None)
def encoded(kind):
    """The corpus as its index kind stores it (numpy; bf16 as uint16 bits) -> (tokens, second or None)."""
    c = corpus(kind)
    if kind == "mxfp8":
        return orc.mxfp8_quantize(c.docs_f32())
    hi = orc.to_bf16_bits(c.dhi / float(ex.ONE))
    assert np.array_equal(pd.decode_bf16(hi).astype(np.float64) * ex.ONE, c.dhi)
    return hi, (orc.to_bf16_bits(c.dlo / float(ex.ONE)) if kind == "fp32" else None)


def _decoded(kind, tok, second):
    """float32 (hi, lo) of the stored arrays, NaN and Inf as the formats decode them."""
    if kind == "mxfp8":
        return pd.decode_mxfp8(tok, second), None
    return pd.decode_bf16(tok), (pd.decode_bf16(second) if kind == "fp32" else None)


def _pad_mask(doclens, ld):
    return np.arange(ld)[None, :] >= np.clip(doclens, 0, ld)[:, None]


# ---------------------------------------------------------------------------- (a) the poisoner
def _synthetic(kind, ld, seed=0):
    """Random finite arrays of an index kind with every doc length the kernels tell apart."""
    rng = np.random.default_rng([seed, ld])
    doclens = np.array([0, ld] + list(range(1, 34)) + [ld - 1, ld - 15, ld - 16, ld - 17, -3, ld + 5], np.int32)
    n = len(doclens)
    if kind == "mxfp8":
        tok = rng.integers(0, 0x7E, (n, ld, ex.DIM)).astype(np.uint8)
        return tok, rng.integers(120, 130, (n, ld, 2)).astype(np.uint8), doclens
    tok = orc.to_bf16_bits(rng.standard_normal((n, ld, ex.DIM)).astype(np.float32))
    second = orc.to_bf16_bits(rng.standard_normal((n, ld, ex.DIM)).astype(np.float32) / 256) if kind == "fp32" else None
    return tok, second, doclens


def _as_torch(kind, a):
    if a is None:
        return None
    return torch.from_numpy(a.copy()) if a.dtype == np.uint8 else torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16)


def _bits(t):
    return t.numpy() if t.dtype == torch.uint8 else t.view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("mode", pd.MODES)
@pytest.mark.parametrize("ld", [128, 256])
@pytest.mark.parametrize("kind", ex.KINDS)
def test_poisoner_overwrites_exactly_the_padding_rows(kind, ld, mode):
    tok, second, doclens = _synthetic(kind, ld)
    keep = [tok.copy(), None if second is None else second.copy()]
    ptok, psecond = pd.poison(kind, tok, second, doclens, mode)
    assert np.array_equal(tok, keep[0]) and (second is None or np.array_equal(second, keep[1]))   # clones
    pad = _pad_mask(doclens, ld)
    assert set((np.clip(doclens, 0, ld) % 16).tolist()) == set(range(16)) and pad[-2].all() and not pad[-1].any()
    for new, old in ((ptok, tok), (psecond, second)):
        if old is None:
            assert new is None
            continue
        assert np.array_equal(new[~pad], old[~pad])                       # every scoring row bit for bit
        assert (new[pad] != old[pad]).any(axis=1).all()                   # every padding row changed
    # torch tensors get the same bytes
    ttok, tsecond = pd.poison(kind, _as_torch(kind, tok), _as_torch(kind, second), torch.from_numpy(doclens), mode)
    assert np.array_equal(_bits(ttok), ptok) and (second is None or np.array_equal(_bits(tsecond), psecond))
    # what the padding decodes to
    hi, lo = _decoded(kind, ptok, psecond)
    rows = hi[pad]                                                        # [padding rows, 128]
    if mode == "nan":
        assert np.isnan(rows).all() and (lo is None or np.isnan(lo[pad]).all())
    else:
        big = np.abs(rows.astype(np.float64)) >= 2.0 ** 127               # the largest finite bf16 magnitudes
        assert (~np.isfinite(rows) | big).all()
        assert np.isinf(rows).any() and (rows == np.inf).any() and (rows == -np.inf).any()
        with np.errstate(over="ignore", invalid="ignore"):
            assert not np.isfinite((rows * rows).sum(axis=1, dtype=np.float32)).any()   # a dot product overflows fp32
        assert lo is None or (~np.isfinite(lo[pad]) | (np.abs(lo[pad].astype(np.float64)) >= 2.0 ** 127)).all()
    if kind == "mxfp8":
        bytes_seen = set(zip(ptok[pad][:, 0].tolist(), psecond[pad][:, 0].tolist()))
        assert bytes_seen == set(zip(pd.E4M3[mode], pd.E8M0[mode]))
        assert mode == "nan" or (0x38, 0xFF) in bytes_seen                # finite bytes, the scale alone NaN
    else:
        assert set(np.unique(ptok[pad]).tolist()) == set(pd.BF16[mode])
    # several patterns inside one partly filled 16-row tile
    i = int(np.nonzero(doclens == 17)[0][0])
    assert len({int(x) for x in ptok[i, 17:32, 0]}) >= 2


@pytest.mark.parametrize("mode", pd.MODES)
def test_f32_poisoner(mode):
    rng = np.random.default_rng(3)
    _, _, doclens = _synthetic("bf16", 128)
    x = rng.standard_normal((len(doclens), 128, ex.DIM)).astype(np.float32)
    p = pd.poison_f32(x, doclens, mode)
    pad = _pad_mask(doclens, 128)
    assert np.array_equal(p[~pad].view(np.uint32), x[~pad].view(np.uint32))
    assert set(np.unique(p[pad].view(np.uint32)).tolist()) == set(pd.F32[mode])
    assert np.isnan(p[pad]).all() if mode == "nan" else (np.isinf(p[pad]).any() and not np.isnan(p[pad]).any())
    t = pd.poison_f32(torch.from_numpy(x), torch.from_numpy(doclens), mode)
    assert np.array_equal(t.numpy().view(np.uint32), p.view(np.uint32))
    # the split of a poisoned matrix: the oracle's scoring rows and bounds are the clean ones
    with np.errstate(all="ignore"):
        hi, lo, bounds = orc.split_f32(p, doclens)
    chi, clo, cbounds = orc.split_f32(x, doclens)
    assert np.array_equal(hi[~pad], chi[~pad]) and np.array_equal(lo[~pad], clo[~pad]) and bounds == cbounds


@pytest.mark.parametrize("kind", ex.KINDS)
def test_query_tail_patterns(kind):
    for mode in pd.MODES:
        a = pd.query_tail(kind, mode, 4096 + 256)
        assert a.dtype == np.uint8 and a.shape == (4096 + 256,)
        if kind == "mxfp8":
            assert set(a.tolist()) <= {0xFE, 0xFF} and not np.isfinite(pd.decode_mxfp8(a[:128], a[128:130])).any()
        else:
            v = a.view(np.uint32).view(np.float32) if kind == "fp32" else pd.decode_bf16(a.view(np.uint16))
            assert np.isnan(v).all() if mode == "nan" else (np.abs(v.astype(np.float64)) >= 2.0 ** 127).all()


# ---------------------------------------------------------------------------- (b), (c) the reference and the leak
def _brute(kind, hi, lo, c, mask, fold):
    """Scores float64 [NQ, N] of decoded arrays.  Per doc the rows of its
    ceil(doclens / 16) tiles take part, as in the kernels.  mask "select": a
    padding row's value is replaced by -inf; "additive": the row's accumulator
    starts at -inf and the products are added on top.  fold: np.maximum (keeps
    a NaN) or np.fmax (drops it), starting from -inf."""
    qh = (c.qhi[:NQ] / float(ex.ONE)).reshape(-1, ex.DIM)
    ql = (c.qlo[:NQ] / float(ex.ONE)).reshape(-1, ex.DIM)
    out = np.empty((NQ, c.N))
    with np.errstate(all="ignore"):
        for i in range(c.N):
            dl = int(c.doclens[i])
            rows = 16 * ((dl + 15) // 16)
            h = hi[i, :rows].astype(np.float64)
            d = h @ qh.T                                                   # [rows, NQ * 32]
            if kind == "fp32":
                d = lo[i, :rows].astype(np.float64) @ qh.T + h @ ql.T + d
            valid = (np.arange(rows) < dl)[:, None]
            d = np.where(valid, d, -np.inf) if mask == "select" else np.where(valid, 0.0, -np.inf) + d
            m = fold.reduce(d, axis=0, initial=-np.inf)
            out[:, i] = m.reshape(NQ, ex.LQ).sum(axis=1)
    return out


def _same(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("kind", ex.KINDS)
def test_reference_ignores_padding_and_the_comparison_sees_a_leak(kind):
    c = corpus(kind)
    tok, second = encoded(kind)
    want = c.ref[:NQ, ex.LQ - 1]
    pad = _pad_mask(c.doclens, c.ld)
    hi, lo = _decoded(kind, tok, second)
    assert np.array_equal(_brute(kind, hi, lo, c, "select", np.maximum), want)        # the scorer itself
    assert np.array_equal(_brute(kind, hi, lo, c, "additive", np.maximum), want)      # finite padding: nothing to leak
    partial = c.doclens % 16 != 0
    assert set((c.doclens[partial] % 16).tolist()) == set(range(1, 16))
    for mode in pd.MODES:
        ptok, psecond = pd.poison(kind, tok, second, c.doclens, mode)
        assert np.array_equal(ptok[~pad], tok[~pad]) and (second is None or np.array_equal(psecond[~pad], second[~pad]))
        hi, lo = _decoded(kind, ptok, psecond)
        # (b) a function of the scoring rows only: the poisoned corpus has the clean reference
        assert np.array_equal(_brute(kind, hi, lo, c, "select", np.maximum), want), mode
        # (c) additive masking is right exactly as long as every fold drops the NaN ...
        assert np.array_equal(_brute(kind, hi, lo, c, "additive", np.fmax), want), mode
        # ... and a fold that keeps it shows in a doc of every partly filled tile class, never elsewhere
        leak = _brute(kind, hi, lo, c, "additive", np.maximum)
        differs = ~_same(leak, want).all(axis=0)
        assert not differs[~partial].any()
        for r in range(1, 16):
            assert differs[c.doclens % 16 == r].any(), (mode, r)
        assert np.isnan(leak[:, differs]).any()


# ---------------------------------------------------------------------------- (d) the replayed walks
def _coverage(kind, ld, seeds):
    eps, values = set(), set()
    for mode in ws.PADDING_MODES:
        for key in ws.padding_walks(kind, ld, mode, seeds):
            for st in wk.generate(*key).steps:
                if st["ep"] not in ("set_options", "invalid"):
                    eps.add(st["ep"])
                    values |= set(zip(wk.OPT_NAMES, st["opts"]))
    return eps, values


CASES = [(kind, ld) for kind in ex.KINDS for ld in wk.LDS]


@pytest.mark.parametrize("kind,ld", CASES, ids=[f"{k}-{ld}" for k, ld in CASES])
def test_padding_walks_cover_every_entry_point_and_option_value(kind, ld):
    want_eps = set(wk.COMMON_EPS + (wk.FAITHFUL_EPS if kind == "fp32" else wk.PLAIN_EPS))
    want_values = {(name, v) for name, _, vals in wk.OPTIONS for v in vals}
    n = ws.PADDING_SEEDS[kind, ld]
    assert n <= ws.SEEDS[kind]                                             # a prefix of the committed walks
    eps, values = _coverage(kind, ld, None)
    assert eps == want_eps and values == want_values
    eps, values = _coverage(kind, ld, {(kind, ld): n - 1})                 # the smallest such prefix
    assert eps != want_eps or values != want_values
    played = [key for mode in ws.PADDING_MODES for key in ws.padding_walks(kind, ld, mode)]
    assert sorted(played) == ws.committed()[ws.committed().index((kind, ld, 0, False)):][:n]
    assert all(ws.padding_walks(kind, ld, mode) for mode in ws.PADDING_MODES)
    assert ws.PADDING_LARGE <= min(ws.LARGE_SEEDS.values())
