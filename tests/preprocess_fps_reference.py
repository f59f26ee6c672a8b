"""The frame-rate filter as a literal queue, shared by tests/test_preprocess_fps_host.py and tests/test_gpu_preprocess_fps.py.

``simulate`` walks ffmpeg's ``fps`` filter (``round=near``, ``eof_action=round``) the way the filter itself runs: a queue of at most
two frames and an output tick.  While the newer frame has reached the tick the older one is dropped; otherwise the older one is
emitted and the tick advances; at the end the last frame is emitted up to the rounded end time.  It shares no code with
``vaura_amd.preprocess.fps_plan`` (a closed form over all frames) and does its own rounding.  Also here: the issue's known answers, the
seeded timestamp generators and the source frame counts both test files use."""
import math
import random
from fractions import Fraction

RATES = {"25": Fraction(25), "30": Fraction(30), "24": Fraction(24), "60": Fraction(60), "50": Fraction(50), "15": Fraction(15),
         "25/2": Fraction(25, 2), "30000/1001": Fraction(30000, 1001), "24000/1001": Fraction(24000, 1001)}

# (frames, rate) -> (N_out, how the selection begins), computed with exact rationals by hand
KNOWN = [
    (32, Fraction(25), 32, list(range(32))),
    (39, Fraction(30), 33, [0, 1, 2, 4, 5, 6, 7, 8, 10]),
    (39, Fraction(30000, 1001), 33, [0, 1, 2, 4, 5, 6, 7, 8, 10]),
    (31, Fraction(24), 32, list(range(12)) + [11, 12]),
    (77, Fraction(60), 32, [1, 3, 5, 8, 10, 13, 15, 17, 20]),
    (16, Fraction(25, 2), 32, [i // 2 for i in range(32)]),
    (20, Fraction(30), 17, [0, 1, 2, 4, 5]),
]
DROPPED_39_AT_30 = [3, 9, 15, 21, 27, 33]

# source frames that give 32 or 33 output frames (2 segments of 16), per rate the GPU tests run
GPU_CASES = [("30", 39, Fraction(30)), ("30000/1001", 39, Fraction(30000, 1001)), ("24", 31, Fraction(24)), ("60", 77, Fraction(60)),
             ("25/2", 16, Fraction(25, 2))]


def round_half_away(x: Fraction) -> int:
    return math.floor(x + Fraction(1, 2)) if x >= 0 else -math.floor(-x + Fraction(1, 2))


def simulate(times, t_end, dst_fps=Fraction(25)):
    """times: the frames' times (Fractions, increasing); t_end: the end of the video -> (first tick, [source frame per output])."""
    queue, out, tick, first = [], [], None, 0
    for i, t in enumerate(times):
        r = round_half_away(t * dst_fps)
        if tick is None:
            tick = first = r
        queue.append((i, r))
        while len(queue) == 2:
            if queue[1][1] <= tick:                                     # the newer frame has reached the tick: the older one is dropped
                queue.pop(0)
            else:                                                       # the older one is shown at this tick
                out.append(queue[0][0])
                tick += 1
    if queue:                                                           # flush: the last frame up to the rounded end
        r_end = round_half_away(t_end * dst_fps)
        while tick < r_end:
            out.append(queue[0][0])
            tick += 1
    return first, out


def simulate_constant(n, src_fps, dst_fps=Fraction(25)):
    return simulate([Fraction(i) / src_fps for i in range(n)], Fraction(n) / src_fps, dst_fps)


def simulate_pts(pts, time_base, end=None, dst_fps=Fraction(25)):
    ts = [p * time_base for p in pts]
    if end is not None:
        t_end = end * time_base
    elif len(ts) >= 2:
        t_end = ts[-1] + (ts[-1] - ts[-2])
    else:
        t_end = ts[0] + 1 / dst_fps
    return simulate(ts, t_end, dst_fps)


def jittered_pts(n, fps, seed, time_base=Fraction(1, 90000), jitter=0.4):
    """A nominally constant rate whose timestamps wobble by up to ``jitter`` of a frame (a camera's clock), strictly increasing."""
    rng = random.Random(seed)
    step = 1 / (fps * time_base)
    pts, last = [], None
    for i in range(n):
        p = int(round(float(step) * (i + rng.uniform(-jitter, jitter))))
        p = p if last is None or p > last else last + 1
        pts.append(p)
        last = p
    return pts


def variable_pts(n, seed, time_base=Fraction(1, 1000)):
    """A variable rate: gaps between 5 and 120 ms, drawn per frame; starts at a non-zero pts."""
    rng = random.Random(seed)
    pts, p = [], rng.randrange(0, 500)
    for _ in range(n):
        pts.append(p)
        p += rng.randrange(5, 121)
    return pts
