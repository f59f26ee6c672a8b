"""fp64 restatement of the packed codec pass (vaura_dac_decode_clips / vaura_dac_encode_clips) on the CPU: the clips of a batch laid
out behind one another as ONE sequence with ``gap`` latent frames between neighbours, every layer run on that sequence as a batch of
one, and the gap rows of every Snake output cleared before a conv with more than one tap reads it.  Built from oracle.dac_oracle's
``fold`` / ``snake`` / ``from_codes`` and its layer order.  With ``gap`` large enough a clip's rows are what the oracle gives for the
clip alone; with ``gap = 0`` the neighbours leak into each other, which the test that uses this must see.

The oracle casts its weights with ``.float()``; ``f64_state_dict`` hands it tensors whose ``.float()`` keeps fp64, so that the oracle
itself — unedited — is the fp64 reference of a clip alone."""
import math

import torch
import torch.nn.functional as F

from oracle import dac_oracle as O


class F64(torch.Tensor):
    """An fp64 tensor that stays fp64 under ``.float()`` (results of torch functions on it are F64 again)."""

    def float(self):
        return self


def f64_state_dict(sd):
    return {k: v.double().as_subclass(F64) for k, v in sd.items()}


def layout(frames, gap):
    offsets, o = [], 0
    for f in frames:
        offsets.append(o)
        o += f + gap
    return offsets, o - gap


def _mask(frames, offsets, total, rate):
    """(1, 1, total * rate): 1 on the rows of a clip, 0 in the gaps."""
    m = torch.zeros(total * rate, dtype=torch.float64)
    for f, o in zip(frames, offsets):
        m[o * rate:(o + f) * rate] = 1
    return m[None, None]


def packed_decode(sd, codes, rates, dilations, gap):
    """codes: list of (K, T_b) int64 -> list of (T_b * hop,) fp64 samples, decoded in one packed sequence."""
    frames = [int(c.shape[-1]) for c in codes]
    offsets, total = layout(frames, gap)
    mask = lambda rate: _mask(frames, offsets, total, rate)
    packed = torch.zeros(1, codes[0].shape[0], total, dtype=torch.int64)
    for c, o in zip(codes, offsets):
        packed[0, :, o:o + c.shape[-1]] = c
    z = O.from_codes(sd, packed) * mask(1)
    x = F.conv1d(z, O.fold(sd, "decoder.model.0."), sd["decoder.model.0.bias"].float(), padding=3)
    rate = 1
    for b, r in enumerate(rates):
        p = f"decoder.model.{b + 1}.block."
        x = O.snake(x, sd[p + "0.alpha"].float()) * mask(rate)
        x = F.conv_transpose1d(x, O.fold(sd, p + "1."), sd[p + "1.bias"].float(), stride=r, padding=math.ceil(r / 2))
        rate *= r
        for u, d in enumerate(dilations):
            q = p + f"{u + 2}.block."
            y = O.snake(x, sd[q + "0.alpha"].float()) * mask(rate)
            y = F.conv1d(y, O.fold(sd, q + "1."), sd[q + "1.bias"].float(), dilation=d, padding=3 * d)
            y = O.snake(y, sd[q + "2.alpha"].float())           # read by the 1 x 1 conv only: a row for that row
            y = F.conv1d(y, O.fold(sd, q + "3."), sd[q + "3.bias"].float())
            x = x + y
    n = len(rates) + 1
    x = O.snake(x, sd[f"decoder.model.{n}.alpha"].float()) * mask(rate)
    x = torch.tanh(F.conv1d(x, O.fold(sd, f"decoder.model.{n + 1}."), sd[f"decoder.model.{n + 1}.bias"].float(), padding=3))
    return [x[0, 0, o * rate:(o + f) * rate] for f, o in zip(frames, offsets)]


def packed_encode_latent(sd, wavs, rates, dilations, gap):
    """wavs: list of (n_b,) fp64 samples -> list of (latent, ceil(n_b / hop)) fp64 latents, encoded in one packed sequence."""
    hop = int(math.prod(rates))
    frames = [math.ceil(w.shape[-1] / hop) for w in wavs]
    offsets, total = layout(frames, gap)
    mask = lambda rate: _mask(frames, offsets, total, rate)
    x = torch.zeros(1, 1, total * hop, dtype=torch.float64)
    for w, o in zip(wavs, offsets):
        x[0, 0, o * hop:o * hop + w.shape[-1]] = w
    x = F.conv1d(x, O.fold(sd, "encoder.block.0."), sd["encoder.block.0.bias"].float(), padding=3)
    rate = hop
    for b, r in enumerate(rates):
        p = f"encoder.block.{b + 1}.block."
        for u, d in enumerate(dilations):
            q = p + f"{u}.block."
            y = O.snake(x, sd[q + "0.alpha"].float()) * mask(rate)
            y = F.conv1d(y, O.fold(sd, q + "1."), sd[q + "1.bias"].float(), dilation=d, padding=3 * d)
            y = O.snake(y, sd[q + "2.alpha"].float())
            y = F.conv1d(y, O.fold(sd, q + "3."), sd[q + "3.bias"].float())
            x = x + y
        x = O.snake(x, sd[p + "3.alpha"].float()) * mask(rate)
        x = F.conv1d(x, O.fold(sd, p + "4."), sd[p + "4.bias"].float(), stride=r, padding=math.ceil(r / 2))
        rate //= r
    n = len(rates) + 1
    x = O.snake(x, sd[f"encoder.block.{n}.alpha"].float()) * mask(rate)
    z = F.conv1d(x, O.fold(sd, f"encoder.block.{n + 1}."), sd[f"encoder.block.{n + 1}.bias"].float(), padding=1)
    return [z[0, :, o:o + f] for f, o in zip(frames, offsets)]
