"""Live video in, host side (no device): the unbounded chunk schedule against longform.chunk_schedule, the video bound against a walk
over the positions the embed reads, the pieces of chunk 0, the ranges a session releases, the bounded bookkeeping, and what open_live /
push refuse — all pure functions (vaura_amd.live, vaura_amd.clip_params)."""
import ctypes as C

import pytest
import torch

from vaura_amd import _lib as L
from vaura_amd import clip_params as cp
from vaura_amd import live
from vaura_amd.longform import chunk_schedule

K, TPF, TV, SEG = 9, 7, 32, 8
PATTERNS = {"delays_0..8": list(range(K)), "parallel": [0] * K}
BLOCKS = [4, 7, 16, 64]


# ---------------------------------------------------------------------------------------------------------------- the schedule
def test_unbounded_schedule_is_chunk_schedule_for_every_duration():
    plan = live.live_plan()
    assert plan["window"] == 4
    for S in range(5, 37):
        sched = chunk_schedule(0.64 * S)
        assert len(sched) == S - plan["window"] + 1                    # chunk c reads the segments c .. c + 3; the last one ends the video
        assert sched == [live.live_chunk(plan, c) for c in range(len(sched))], S
        assert sched[-1]["max_gen_len"] == plan["full"]                # the last chunk is again a full window
    c0, c1 = live.live_chunk(plan, 0), live.live_chunk(plan, 1)
    assert (c0["max_gen_len"], c0["prompt_len"], c0["positions"]) == (221, 0, (0, 4))
    assert (c1["offset"], c1["max_gen_len"], c1["prompt_len"], c1["new_tokens"], c1["positions"]) == (55, 221, 166, 55, (1, 5))


def test_four_segments_are_the_single_chunk_exception():
    """S = 4 is the single-chunk path with one frame less than chunk 0 of a longer video: not a prefix of it (the tail fix-up of the
    delay pattern differs), so a session closed after four segments is NOT generate_long of 2.56 s — it is chunk 0 of a longer video."""
    (single,) = chunk_schedule(0.64 * 4)
    assert single["positions"] is None and single["max_gen_len"] == 220 == live.live_plan()["first"] - 1


def test_a_stride_that_is_not_one_segment_is_refused():
    with pytest.raises(L.VauraHipError, match="one 16-frame segment per chunk"):
        live.live_plan(stride=1.28)
    with pytest.raises(L.VauraHipError, match="one 16-frame segment per chunk"):
        live.live_plan(vfps=30)


# ---------------------------------------------------------------------------------------------------------------- the video bound
def brute_force_bound(V, Tv, tpf, start, S):
    """Walk the positions in the loop's order: the step at position p embeds condition token p // tpf when that is < Tv (csrc/step.hip
    embed_kernel), and may run only when the token has arrived.  Positions 0 .. start - 2 are teacher-forced, sampled step j sits at
    position start - 1 + j; the last position embedded is S - 2 (its step fills slot S - 1)."""
    p = 0
    while p <= S - 2 and (p // tpf >= Tv or p // tpf < V):
        p += 1
    return max(0, p - (start - 1))


@pytest.mark.parametrize("pattern", list(PATTERNS), ids=list(PATTERNS))
def test_video_bound_against_a_walk_over_the_positions(pattern):
    d = PATTERNS[pattern]
    for T in (221, 43, 230):
        S = T + max(d) + 1
        for start in (1 + d[0], 6 + d[0], 167 + d[0]):
            if start > S - 1:
                continue
            for V in range(0, TV + 9):
                assert cp.video_step_bound(V, TV, TPF, start, S) == brute_force_bound(V, TV, TPF, start, S), (T, start, V)
    S = 221 + max(d) + 1
    assert [cp.video_step_bound(8 * i, TV, TPF, 1, S) for i in range(1, 5)] == [56, 112, 168, S - 1]
    for tpf in (1, 3, 7):
        for V in range(0, 12):
            assert cp.video_step_bound(V, 10, tpf, 1, 40) == brute_force_bound(V, 10, tpf, 1, 40)


@pytest.mark.parametrize("block_frames", BLOCKS)
@pytest.mark.parametrize("pattern", list(PATTERNS), ids=list(PATTERNS))
def test_pieces_of_chunk_0(pattern, block_frames):
    d = PATTERNS[pattern]
    T, start = live.live_plan()["first"], 1 + d[0]
    S = T + max(d) + 1
    per_push = cp.live_schedule(T, start, d, block_frames, TPF, TV, SEG)
    assert len(per_push) == TV // SEG
    steps, at = 0, 0
    whole = [0]
    for n, _ in cp.stream_schedule(T, None, start, d, 0, block_frames):
        whole.append(whole[-1] + n)
    for i, pieces in enumerate(per_push):
        bound = cp.video_step_bound(SEG * (i + 1), TV, TPF, start, S)
        for n, (lo, hi) in pieces:
            assert n >= 1 and lo == at and hi >= lo
            steps += n
            at = hi
            assert hi == cp.final_frames(steps, T, start, max(d))      # exactly what is final, no frame held back, none ahead
            assert steps in whole or steps == bound                    # a boundary of stream_schedule, or the cut at the video bound
        assert steps == bound                                          # a push runs everything its video allows, and nothing more
    assert steps == S - start and at == T                              # the pieces sum to the sampled steps of chunk 0


# ---------------------------------------------------------------------------------------------------------------- what a session releases
@pytest.mark.parametrize("block_frames", BLOCKS)
@pytest.mark.parametrize("pattern", list(PATTERNS), ids=list(PATTERNS))
def test_released_ranges_tile_the_frames_in_order(pattern, block_frames):
    plan, H = live.live_plan(), 5
    for S in (1, 2, 3, 4, 5, 6, 9):
        book = live.LiveBook(plan, PATTERNS[pattern], block_frames, TPF, SEG, H)
        at, first = 0, None
        for i in range(S):
            work, rel = book.push()
            assert work[0] == ("steps" if i < plan["window"] else "chunk")
            if rel and first is None:
                first = i
            for lo, hi in rel:
                assert lo == at and hi > lo
                at = hi
        last = book.close()
        assert last is not None and last[0] == at and last[1] - last[0] == min(H, last[1])      # the halo that was held back
        n = last[1]
        want = live.live_chunk(plan, S - plan["window"]) if S >= plan["window"] else None
        if want:
            assert n == want["offset"] + want["max_gen_len"]
        else:
            d_max = max(PATTERNS[pattern])
            assert n == cp.final_frames(cp.video_step_bound(SEG * S, TV, TPF, book.first_step, plan["first"] + d_max + 1), plan["first"],
                                        book.first_step, d_max)
        assert first == 0 or block_frames == 64 and first is not None    # audio is due after ONE segment
        with pytest.raises(L.VauraHipError, match="after close"):
            book.push()


def test_bookkeeping_of_100_segments_is_bounded():
    plan = live.live_plan()
    book = live.LiveBook(plan, PATTERNS["delays_0..8"], 16, TPF, SEG, 5)

    def size(o):
        if isinstance(o, (list, tuple)):
            return 1 + sum(size(x) for x in o)
        if isinstance(o, dict):
            return 1 + sum(size(v) for v in o.values())
        return 1
    sizes, at = [], 0
    for _ in range(100):
        _, rel = book.push()
        at = rel[-1][1] if rel else at
        sizes.append(size(vars(book)))
    assert len(set(sizes)) == 1                                         # not one word more after 100 segments than after one
    assert book.known == 96 * plan["stride_tokens"] + plan["full"] and at == book.known - 5


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_open_live_refusals():
    live.check_open(2, 16)
    for kw, match in [(dict(num_candidates=2), "num_candidates = 1"), (dict(prompt_lengths=[3, 4]), "live clock"),
                      (dict(max_new_tokens=[221, 100]), "live clock"), (dict(video_lengths=[32, 8]), "live clock"),
                      (dict(audio_lengths=[1000, 2000]), "live clock"), (dict(near_tie="rerun"), 'near_tie="rerun"')]:
        with pytest.raises(L.VauraHipError, match=match):
            live.check_open(2, 16, **kw)
    with pytest.raises(L.VauraHipError, match="block_frames"):
        live.check_open(2, 0)
    with pytest.raises(L.VauraHipError, match="batch"):
        live.check_open(0, 16)


def test_push_refusals():
    a = (2, SEG, 768, 16, False)
    assert live.check_push(torch.zeros(2, 1, SEG, 768), None, *a) == "features"
    assert live.check_push(torch.zeros(2, SEG, 768), None, *a) == "features"
    assert live.check_push(None, torch.zeros(2, 1, 3, 16, 2, 2), *a) == "frames"
    for feats in (torch.zeros(2, 4, SEG, 768), torch.zeros(3, SEG, 768), torch.zeros(2, SEG + 1, 768), torch.zeros(2, SEG, 767)):
        with pytest.raises(L.VauraHipError, match="one segment is"):
            live.check_push(feats, None, *a)
    for frames in (torch.zeros(2, 2, 3, 16, 2, 2), torch.zeros(2, 1, 3, 8, 2, 2), torch.zeros(2, 3, 16, 2, 2)):
        with pytest.raises(L.VauraHipError, match="one segment is"):
            live.check_push(None, frames, *a)
    with pytest.raises(L.VauraHipError, match="not both and not neither"):
        live.check_push(None, None, *a)
    with pytest.raises(L.VauraHipError, match="not both and not neither"):
        live.check_push(torch.zeros(2, SEG, 768), torch.zeros(2, 1, 3, 16, 2, 2), *a)
    with pytest.raises(L.VauraHipError, match="after close"):
        live.check_push(torch.zeros(2, SEG, 768), None, 2, SEG, 768, 16, True)


def test_cond_window_argument_errors_without_a_gpu():
    lib = L.lib()
    assert "vaura_cond_window" in L.SIGNATURES
    assert lib.vaura_cond_window(None, 0, 0, 0, 0, 8, 0) == -1          # VAURA_ERR_ARG: no descriptor
    d = L.Decoder()
    assert lib.vaura_cond_window(C.byref(d), 0, 0, 0, 0, 8, 0) == -1    # no condition buffer
