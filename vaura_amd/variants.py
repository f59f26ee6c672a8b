"""Kernel-variant switches of libvaura_hip by name: the Python mirror of vaura_amd/csrc/variants.h (the table; what each switch does
is written there, tests/test_variants_host.py holds the two together).  Variant is the word of vaura_set_debug_flags, Variant2 the
word of vaura_set_debug_flags2; the product runs with both 0.

    with variants(Variant.CODEC_UNIT_TWO_LAUNCHES):            # both words set here ...
        two = dec.decode(codes)
    ...                                                        # ... and both 0 again, also after an exception

The words are process-global, so a block that is entered while another one is open would switch the outer block's variant off when it
ends: variants() refuses to nest (RuntimeError, nothing changed).  Combine switches in one call: variants(A | B, Variant2.C).
"""
from __future__ import annotations

import contextlib
import enum
import os


class Variant(enum.IntFlag):
    ROWSPLIT_OFF = 1 << 0
    QKV_OWN_LAUNCH = 1 << 1
    MLP_TWO_LAUNCHES = 1 << 2
    PREFILL_ATTN_PER_POSITION = 1 << 4
    PREFILL_GEMM_64_ROWS = 1 << 5
    VIT_SPACE_THREAD_PER_QUERY = 1 << 7
    VIT_CLS_UNSPLIT = 1 << 9
    VIT_TIME_THREAD_PER_HEAD_FRAME = 1 << 10
    VIT_SPACE_FP32_MFMA = 1 << 11
    CODEC_LAST_CONV_UNTILED = 1 << 13
    GEMM3_ROUND2_TILE_RULE = 1 << 14
    PREFILL_GEMM_LAUNCH_ORDER = 1 << 15
    GEMM3_ONE_KGROUP = 1 << 16
    PREFILL_GEMM_REGISTER_STAGED = 1 << 17
    GEMM4_NO_DMA = 1 << 18
    ATTN_MERGE_OWN_LAUNCH = 1 << 19
    CODEC_128_ROWS = 1 << 20
    CODEC_UNIT_TWO_LAUNCHES = 1 << 21
    PREFILL_GEMM_NO_CUT = 1 << 22
    PREFILL_GEMM_64x256 = 1 << 23


class Variant2(enum.IntFlag):
    ROW_BLOCKS_WALK = 1 << 0
    ENGINE_MAX_16_ROWS = 1 << 1
    FP8_ROWSPLIT_OFF = 1 << 3
    FP8_NO_ENGINE = 1 << 4
    LINEAR_REGISTER_STAGED = 1 << 5
    LINEAR_DMA_LATE_FRAGMENTS = 1 << 6


FIELDS = {"GRAPH_STEPS": (1, 24, 4), "ENGINE_ABL": (1, 28, 4), "LINEAR_PANEL": (2, 12, 4)}      # name: (word, shift, width)


def _field(name: str, n: int) -> int:
    _, shift, width = FIELDS[name]
    if not 0 <= n < (1 << width):
        raise ValueError(f"{name} takes 0..{(1 << width) - 1}, not {n}")
    return n << shift


def graph_steps(n: int) -> int:
    """word 1: decode steps per graph launch"""
    return _field("GRAPH_STEPS", n)


def engine_abl(n: int) -> int:
    """word 1: timing ablations of the one-launch MLP"""
    return _field("ENGINE_ABL", n)


def linear_panel(n: int) -> int:
    """word 2: column-tile panel of the extractor's linear layers"""
    return _field("LINEAR_PANEL", n)


_open = False


@contextlib.contextmanager
def variants(word1: int = 0, word2: int = 0, lib=None):
    """Run the block under these two words; both are 0 afterwards, whatever ends the block."""
    global _open
    if _open:
        raise RuntimeError("variants() does not nest: the words are process-global (pass every switch to one call)")
    if lib is None:
        from . import _lib
        lib = _lib.lib()
    _open = True
    try:
        lib.vaura_set_debug_flags(int(word1))
        lib.vaura_set_debug_flags2(int(word2))
        yield
    finally:
        lib.vaura_set_debug_flags(0)
        lib.vaura_set_debug_flags2(0)
        _open = False


def parse(text: str, names=Variant) -> int:
    """one word from text: integers (any base prefix) or switch names of `names`, joined by | or ,"""
    word = 0
    for part in text.replace(",", "|").split("|"):
        part = part.strip()
        if part:
            word |= int(names[part]) if part in names.__members__ else int(part, 0)
    return word


def from_env(environ=None):
    """(word1, word2) from VAURA_DEBUG_FLAGS / VAURA_DEBUG_FLAGS2, each as parse() reads it"""
    e = os.environ if environ is None else environ
    return parse(e.get("VAURA_DEBUG_FLAGS", "0"), Variant), parse(e.get("VAURA_DEBUG_FLAGS2", "0"), Variant2)
