"""Non-finite padding rows (test infrastructure): the poisoner of an index's
padding, beside tests/_exact.py.

The header promises that rows t >= doclens[i] of a doc never score and that no
value outside the stated extents influences a result.  The library borrows the
caller's arrays, so a caller that allocates without clearing, or fills with
0xFF bytes, hands it NaN and Inf encodings there.  ``poison`` writes such
encodings into exactly the padding rows of CLONES of an index's arrays, as the
library stores them, and touches nothing else; the exact reference of
tests/_exact.py is a function of the scoring rows only, so every expected
score stays what it was.

Works on numpy arrays and on torch tensors (CPU or GPU) alike: everything is
done on integer views of the arrays' bits.  numpy holds bf16 as uint16.

Patterns cycle with (doc + row), so one 16-row tile holds several of a mode:
  bf16 tokens / residual (and the faithful index's hi / lo, written directly)
    nan   0x7FC0 qNaN, 0x7F81 sNaN, 0xFFFF (a 0xFF byte fill)
    inf   0x7F80 +Inf, 0xFF80 -Inf, 0x7F7F / 0xFF7F the largest finite
          magnitudes (their dot products overflow fp32)
  MXFP8 (e4m3 byte of the whole row, both scale bytes)
    nan   (0x7F, 0xFF), (0xFF, 0xFF)
    inf   (0x7E, 0xFE), (0xFE, 0xFF), (0x7E, 0xFF), (0xFE, 0xFE): +-448 under
          the scales 2^127 and NaN; (0x38, 0xFF): finite bytes (1.0) whose
          scale alone is 0xFF
  f32 (the source matrix of cbv2_split_f32 / cbv2_index_build_means)
    nan   0x7FC00000 qNaN, 0x7F800001 sNaN, 0xFFFFFFFF
    inf   0x7F800000 +Inf, 0xFF800000 -Inf, 0x7F7FFFFF / 0xFF7FFFFF
The residual of a row takes the pattern after its tokens' one.
"""
import numpy as np

MODES = ("nan", "inf")
BF16 = {"nan": (0x7FC0, 0x7F81, 0xFFFF), "inf": (0x7F80, 0xFF80, 0x7F7F, 0xFF7F)}
F32 = {"nan": (0x7FC00000, 0x7F800001, 0xFFFFFFFF), "inf": (0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF)}
E4M3 = {"nan": (0x7F, 0xFF), "inf": (0x7E, 0xFE, 0x7E, 0xFE, 0x38)}
E8M0 = {"nan": (0xFF, 0xFF), "inf": (0xFE, 0xFF, 0xFF, 0xFE, 0xFF)}
_UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32}
_SINT = {1: np.uint8, 2: np.int16, 4: np.int32}          # torch has no unsigned 16 / 32-bit views


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def clone(x):
    return x.clone() if _is_torch(x) else x.copy()


def padding_rows(doclens, ld, like=None):
    """(doc, row) of every padding row, in row-major order, as index arrays of
    ``like``'s library and device; doclens clamped to [0, ld] as the library
    clamps them."""
    if like is not None and _is_torch(like):
        import torch
        dl = torch.as_tensor(doclens).to(like.device).long().clamp(0, ld)
        pad = torch.arange(ld, device=like.device)[None, :] >= dl[:, None]
        return pad.nonzero(as_tuple=True)
    dl = np.clip(np.asarray(doclens).astype(np.int64), 0, ld)
    return np.nonzero(np.arange(ld)[None, :] >= dl[:, None])


def _write(arr, doclens, patterns, shift=0):
    """Pattern (doc + row + shift) mod len into every element of every padding
    row of ``arr`` [n, ld, w], in place, through its bits."""
    n, ld, _ = arr.shape
    size = arr.element_size() if _is_torch(arr) else arr.dtype.itemsize
    i, t = padding_rows(doclens, ld, arr)
    if _is_torch(arr):
        import torch
        table = torch.from_numpy(np.array(patterns, _UINT[size]).view(_SINT[size])).to(arr.device)
        bits = arr.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[size])
        bits[i, t] = table[(i + t + shift) % len(patterns)][:, None]
    else:
        table = np.array(patterns, _UINT[size])
        arr.view(_UINT[size])[i, t] = table[(i + t + shift) % len(patterns)][:, None]
    return arr


def poison(kind, tokens, second, doclens, mode):
    """Clones of an index's arrays with every padding row overwritten:
    ``tokens`` bf16 [n, ld, 128] (uint16 in numpy) or the e4m3 bytes, ``second``
    the bf16 residual ("fp32"), the E8M0 scales [n, ld, 2] ("mxfp8") or None
    ("bf16") -> (tokens, second)."""
    assert mode in MODES and kind in ("bf16", "mxfp8", "fp32")
    tok = _write(clone(tokens), doclens, E4M3[mode] if kind == "mxfp8" else BF16[mode])
    if kind == "bf16":
        assert second is None
        return tok, None
    return tok, _write(clone(second), doclens, E8M0[mode] if kind == "mxfp8" else BF16[mode], shift=kind == "fp32")


def poison_f32(x, doclens, mode):
    """A clone of an f32 matrix [n, ld, 128] with every padding row overwritten."""
    assert mode in MODES
    return _write(clone(x), doclens, F32[mode])


def query_tail(kind, mode, nbytes):
    """uint8 [nbytes]: what a walk's query buffer holds past the step's
    queries.  A bf16 / f32 buffer holds the mode's values; the quantised MXFP8
    layout (e4m3 rows, then their scale bytes) holds bytes that are non-finite
    both as an e4m3 value and as a scale: 0xFF (NaN, NaN) or 0xFE (-448, 2^127)
    and 0xFF by turns of 128."""
    if kind == "mxfp8":
        row = np.arange(nbytes) // 128
        return np.where(row % 2 == 0, 0xFF if mode == "nan" else 0xFE, 0xFF).astype(np.uint8)
    table = np.array(F32[mode], np.uint32) if kind == "fp32" else np.array(BF16[mode], np.uint16)
    per = 128 * table.dtype.itemsize                                       # one pattern per query row
    rows = table[np.arange((nbytes + per - 1) // per) % len(table)]
    return np.repeat(rows, 128).view(np.uint8)[:nbytes].copy()


# ---------------------------------------------------------------------------- decoding (the CPU tests)
def decode_bf16(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def decode_mxfp8(q, scales):
    """float32 values of e4m3 bytes [..., 128] under E8M0 scales [..., 2]: 0x7F /
    0xFF bytes and a 0xFF scale are NaN, +-448 * 2^127 overflows to +-Inf."""
    from oracle import oracle as orc
    s = np.asarray(scales, np.float64)
    mult = np.where(s == 255, np.nan, np.exp2(s - 127.0))
    with np.errstate(over="ignore", invalid="ignore"):
        return (orc.E4M3[np.asarray(q, np.uint8)] * np.repeat(mult, 64, axis=-1)).astype(np.float32)
