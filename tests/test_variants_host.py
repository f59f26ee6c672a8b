"""The kernel-variant switches (vaura_amd/csrc/variants.h) without a GPU: the header's table and vaura_amd/variants.py name the same
bits, no two switches share one, nothing in csrc/ reads the two words except through the header, and variants() always puts both
words back to 0."""
import glob
import os
import re

import pytest

from vaura_amd import variants as V

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vaura_amd", "csrc")
SWITCH = re.compile(r'^\s*X\((\w+), ([12]), (\d+), "')
FIELD = re.compile(r'^\s*X\((\w+), ([12]), (\d+), (\d+), "')


def _table():
    switches, fields = {}, {}
    for line in open(os.path.join(CSRC, "variants.h")):
        if (m := FIELD.match(line)):
            assert m.group(1) not in fields, m.group(1)
            fields[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
        elif (m := SWITCH.match(line)):
            assert m.group(1) not in switches, m.group(1)
            switches[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    return switches, fields


def test_header_and_python_name_the_same_bits():
    switches, fields = _table()
    assert len(switches) >= 26 and len(fields) == 3
    py = {m.name: (word, m.value) for word, enum in ((1, V.Variant), (2, V.Variant2)) for m in enum}
    assert py == {name: (word, 1 << bit) for name, (word, bit) in switches.items()}
    assert V.FIELDS == fields
    for name, (word, shift, width) in fields.items():
        helper = getattr(V, name.lower())
        top = (1 << width) - 1
        assert helper(0) == 0 and helper(1) == 1 << shift and helper(top) == top << shift
        with pytest.raises(ValueError):
            helper(top + 1)


def test_no_two_entries_share_a_bit():
    switches, fields = _table()
    seen = {1: 0, 2: 0}
    for name, (word, bit) in switches.items():
        assert 0 <= bit < 32 and not seen[word] >> bit & 1, name
        seen[word] |= 1 << bit
    for name, (word, shift, width) in fields.items():
        mask = ((1 << width) - 1) << shift
        assert width >= 1 and shift + width <= 32 and not seen[word] & mask, name
        seen[word] |= mask
    # the values the committed records and tools/pmc_driver --flags were taken with
    assert seen == {1: 0xFFFFFFFF & ~(1 << 3 | 1 << 6 | 1 << 8 | 1 << 12), 2: 0b1111_0000_0111_1011}


# the only lines that may name the words: their definitions, getters and exported setters (gemv3.hip)
DEFINITIONS = {
    "unsigned va_debug_flags = 0;",
    "unsigned va_debug_flags2 = 0;",
    "unsigned va_debug_flags_get() { return va_debug_flags; }",
    "unsigned va_debug_flags2_get() { return va_debug_flags2; }",
    'extern "C" void vaura_set_debug_flags(unsigned flags) { va_debug_flags = flags; }',
    'extern "C" void vaura_set_debug_flags2(unsigned flags) { va_debug_flags2 = flags; }',
}


def test_nothing_in_csrc_reads_the_words_past_the_header():
    sources = [p for ext in ("*.hip", "*.h", "*.cpp", "*.hpp") for p in glob.glob(os.path.join(CSRC, ext))]
    assert len(sources) > 12
    found = set()
    for path in sources:
        if os.path.basename(path) == "variants.h":
            continue
        for n, line in enumerate(open(path), 1):
            if re.search(r"\bva_debug_flags2?(_get)?\b", line):
                assert os.path.basename(path) == "gemv3.hip" and line.strip() in DEFINITIONS, f"{os.path.basename(path)}:{n}: {line.strip()}"
                found.add(line.strip())
    assert found == DEFINITIONS


class StubLib:
    def __init__(self):
        self.words, self.calls = [None, None], []

    def vaura_set_debug_flags(self, w):
        self.words[0] = w
        self.calls.append((1, w))

    def vaura_set_debug_flags2(self, w):
        self.words[1] = w
        self.calls.append((2, w))


def test_variants_sets_both_words_and_always_puts_back_zero():
    lib = StubLib()
    with V.variants(V.Variant.CODEC_128_ROWS | V.graph_steps(2), V.Variant2.ROW_BLOCKS_WALK, lib=lib):
        assert lib.words == [1 << 20 | 2 << 24, 1] and all(type(w) is int for w in lib.words)
    assert lib.words == [0, 0]
    with V.variants(word2=V.linear_panel(15), lib=lib):
        assert lib.words == [0, 15 << 12]
    assert lib.words == [0, 0]
    with pytest.raises(KeyError):
        with V.variants(V.Variant.MLP_TWO_LAUNCHES, lib=lib):
            assert lib.words == [4, 0]
            raise KeyError("inside the block")
    assert lib.words == [0, 0]


def test_variants_refuses_to_nest():
    lib = StubLib()
    with V.variants(V.Variant.QKV_OWN_LAUNCH, lib=lib):
        n = len(lib.calls)
        with pytest.raises(RuntimeError):
            with V.variants(V.Variant.MLP_TWO_LAUNCHES, lib=lib):
                pass
        assert lib.words == [2, 0] and len(lib.calls) == n      # the refused block changed nothing
    assert lib.words == [0, 0]
    with V.variants(lib=lib):                                      # and the refusal left nothing open
        assert lib.words == [0, 0]


def test_from_env_takes_integers_and_names():
    assert V.from_env({}) == (0, 0)
    assert V.from_env({"VAURA_DEBUG_FLAGS": "16", "VAURA_DEBUG_FLAGS2": "32"}) == (16, 32)
    assert V.from_env({"VAURA_DEBUG_FLAGS": "0x20|PREFILL_GEMM_NO_CUT"}) == (32 | 1 << 22, 0)
    assert V.from_env({"VAURA_DEBUG_FLAGS2": "LINEAR_REGISTER_STAGED, 61440"}) == (0, 32 | 15 << 12)
    with pytest.raises(ValueError):
        V.from_env({"VAURA_DEBUG_FLAGS": "NO_SUCH_SWITCH"})
