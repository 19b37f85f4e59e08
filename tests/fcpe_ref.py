"""The FCPE pitch network restated in torch functions (test helper, no GPU needed).

rvc/lib/predictors/FCPE.py, operation by operation: STFT.get_mel / Wav2Mel.extract_mel (:102-168, :790-813), FCPE.forward
(:649-665) with PCmer's layers (:270-283), SelfAttention / FastAttention / softmax_kernel / linear_attention (:462-559,
:399-459, :179-212, :354-363), ConformerConvModule (:327-351), the cents decoders (:683-714) and
FCPEF0Predictor.post_process (:877-902). Like oracle/*.py it follows the dtype of its weights and input, so one
restatement gives the float64 answer and the float32 run whose distance from it anchors the device's bound
(tests/parity_anchor.py). The reference module cannot do that itself: its mel casts the basis to float32 (:126).

`w` is the FCPE module's state dict with dense_out's weight-norm fused (rvcx.weights.check_fcpe_state), `z` the flat
sizes of its config (rvcx.weights.fcpe_sizes).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

HEADS, DIM_HEAD, CONV_K = 8, 64, 31


def mel_basis(z) -> np.ndarray:
    """librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) (htk=False, norm='slaney', float32), FCPE.py:123-126."""
    from oracle.rmvpe import mel_filterbank

    return mel_filterbank(z["sampling_rate"], z["n_fft"], z["num_mels"], z["fmin"], z["fmax"], htk=False)


def n_frames(z, n: int) -> int:
    win, hop = z["win_size"], z["hop_size"]
    pl = (win - hop) // 2
    pr = max((win - hop + 1) // 2, win - n - pl)
    fs = (n + pl + pr - win) // hop + 1
    nf = n // hop + 1
    return fs + 1 if nf > fs else nf


def mel(z, audio: torch.Tensor) -> torch.Tensor:
    """audio [n] -> log-mel [F, num_mels] (get_mel with keyshift 0, center False; extract_mel's frame count)."""
    win, hop = z["win_size"], z["hop_size"]
    n = int(audio.shape[-1])
    pl = (win - hop) // 2
    pr = max((win - hop + 1) // 2, win - n - pl)
    y = F.pad(audio.reshape(1, 1, -1), (pl, pr), mode="reflect" if pr < n else "constant").reshape(1, -1)
    spec = torch.stft(y, n_fft=z["n_fft"], hop_length=hop, win_length=win,
                      window=torch.hann_window(win, dtype=audio.dtype), center=False, normalized=False, onesided=True,
                      return_complex=True)
    spec = torch.sqrt(spec.real.pow(2) + spec.imag.pow(2) + 1e-9)
    # the basis is data: float32-valued in every dtype
    m = torch.matmul(torch.from_numpy(mel_basis(z)).to(audio.dtype), spec)
    m = torch.log(torch.clamp(m, min=1e-5))[0].transpose(0, 1)  # [frames, mels]
    nf = n // hop + 1
    if nf > m.shape[0]:
        m = torch.cat((m, m[-1:]), 0)
    return m[:nf] if nf < m.shape[0] else m


def softmax_kernel(data, proj, is_query: bool, eps: float = 1e-4):
    """FCPE.py:179-212 on data [H, T, D], proj [M, D]."""
    dn = data.shape[-1] ** -0.25
    ratio = proj.shape[0] ** -0.5
    dash = (dn * data) @ proj.to(data.dtype).transpose(0, 1)  # [H, T, M]
    diag = ((data ** 2).sum(-1) / 2.0 * dn ** 2).unsqueeze(-1)
    if is_query:
        return ratio * (torch.exp(dash - diag - dash.max(dim=-1, keepdim=True).values) + eps)
    return ratio * torch.exp(dash - diag + eps)


def dash_minus_diag_k(k, proj):
    """The keys' exponent (without the + eps): the quantity whose maximum the tests bound."""
    dn = k.shape[-1] ** -0.25
    dash = (dn * k) @ proj.to(k.dtype).transpose(0, 1)
    return dash - ((k ** 2).sum(-1) / 2.0 * dn ** 2).unsqueeze(-1)


def performer_attention(q, k, v, proj):
    """FastAttention.forward + linear_attention (FCPE.py:439-459, :354-363): q, k, v [H, T, D] -> [H, T, D]."""
    qp = softmax_kernel(q, proj, True)
    kp = softmax_kernel(k, proj, False)
    ksum = kp.sum(dim=-2)  # [H, M]
    d_inv = 1.0 / ((qp @ ksum.unsqueeze(-1)).squeeze(-1) + 1e-8)  # [H, T]
    ctx = kp.transpose(-1, -2) @ v  # [H, M, D]
    return (qp @ ctx) * d_inv.unsqueeze(-1)


def _layer(w, p, x, taps=None):
    """_EncoderLayer.forward (FCPE.py:280-283) on x [T, C]."""
    C = x.shape[-1]
    h = F.layer_norm(x, (C,), w[p + "norm.weight"], w[p + "norm.bias"])
    q, k, v = (F.linear(h, w[p + f"attn.{n}.weight"], w[p + f"attn.{n}.bias"]).reshape(-1, HEADS, DIM_HEAD)
               .transpose(0, 1) for n in ("to_q", "to_k", "to_v"))
    proj = w[p + "attn.fast_attention.projection_matrix"]
    if taps is not None:
        taps.append((q, k, v, proj))
    o = performer_attention(q, k, v, proj).transpose(0, 1).reshape(-1, HEADS * DIM_HEAD)
    x = x + F.linear(o, w[p + "attn.to_out.weight"], w[p + "attn.to_out.bias"])
    c = p + "conformer.net."
    h = F.layer_norm(x, (C,), w[c + "0.weight"], w[c + "0.bias"]).transpose(0, 1).unsqueeze(0)  # [1, C, T]
    h = F.conv1d(h, w[c + "2.weight"], w[c + "2.bias"])
    a, g = h.chunk(2, dim=1)
    h = a * g.sigmoid()
    pad = CONV_K // 2
    h = F.conv1d(F.pad(h, (pad, pad - (CONV_K + 1) % 2)), w[c + "4.conv.weight"], w[c + "4.conv.bias"],
                 groups=h.shape[1])
    h = h * h.sigmoid()
    h = F.conv1d(h, w[c + "6.weight"], w[c + "6.bias"])
    return x + h[0].transpose(0, 1)


def salience(w, z, m: torch.Tensor, taps=None) -> torch.Tensor:
    """FCPE.forward up to the sigmoid (FCPE.py:657-665): mel [F, num_mels] -> [F, out_dims]."""
    x = m.transpose(0, 1).unsqueeze(0)
    x = F.conv1d(x, w["stack.0.weight"], w["stack.0.bias"], padding=1)
    x = F.leaky_relu(F.group_norm(x, 4, w["stack.1.weight"], w["stack.1.bias"]), 0.01)
    x = F.conv1d(x, w["stack.3.weight"], w["stack.3.bias"], padding=1)[0].transpose(0, 1)
    for i in range(z["n_layers"]):
        x = _layer(w, f"decoder._layers.{i}.", x, taps)
    x = F.layer_norm(x, (x.shape[-1],), w["norm.weight"], w["norm.bias"])
    return torch.sigmoid(F.linear(x, w["dense_out.weight"], w["dense_out.bias"]))


def salience_from_audio(w, z, audio: torch.Tensor, taps=None) -> torch.Tensor:
    return salience(w, z, mel(z, audio), taps)


def decode(y: torch.Tensor, cent_table: torch.Tensor, threshold: float, decoder: str = "local_argmax") -> torch.Tensor:
    """cents_local_decoder / cents_decoder + cent_to_f0 (FCPE.py:683-714) on salience [F, bins] -> f0 [F]."""
    ci = cent_table.to(y.dtype)[None, :].expand(y.shape[0], -1)
    conf, mi = torch.max(y, dim=-1, keepdim=True)
    if decoder == "local_argmax":
        idx = torch.clamp(torch.arange(0, 9) + (mi - 4), 0, y.shape[-1] - 1)
        ci_l, y_l = torch.gather(ci, -1, idx), torch.gather(y, -1, idx)
        rtn = torch.sum(ci_l * y_l, dim=-1, keepdim=True) / torch.sum(y_l, dim=-1, keepdim=True)
    elif decoder == "argmax":
        rtn = torch.sum(ci * y, dim=-1, keepdim=True) / torch.sum(y, dim=-1, keepdim=True)
    else:
        raise ValueError(decoder)
    mask = torch.ones_like(conf)
    mask[conf <= threshold] = float("-inf")
    return (10.0 * 2 ** (rtn * mask / 1200.0))[:, 0]


def post_process(f0, hop: int, sr: int, pad_to=None) -> np.ndarray:
    """FCPEF0Predictor.post_process (FCPE.py:877-902) with compute_f0's all-unvoiced case (:908-909): f0 [F] ->
    float64 [pad_to or F]."""
    f0 = torch.as_tensor(np.asarray(f0)).float()
    n = int(pad_to) if pad_to is not None else int(f0.shape[0])
    if pad_to is not None:
        f0 = F.interpolate(f0[None, None], size=n, mode="nearest")[0, 0]
    nz = torch.nonzero(f0).reshape(-1)
    val = f0[nz].numpy()
    if val.shape[0] == 0:
        return np.zeros(n)
    if val.shape[0] == 1:
        return np.ones(n) * val[0]
    return np.interp(np.arange(n) * hop / sr, hop / sr * nz.numpy(), val, left=val[0], right=val[-1])


# the Performer attention of the kernel-level GPU tests: FCPE's 8 heads of 64 channels, 266 random features
ATTN_H, ATTN_D, ATTN_M = 8, 64, 266


def attention_operands(T, pscale, seed):
    """q, k, v [H][T][64] with element magnitudes spread over two decades (0.03 .. 3 times a unit normal) and a
    gaussian-orthogonal P [266][64] with rows of chi(64) norm. pscale multiplies P's rows; q and k are divided by
    it as well, because dash = c x . P_j would otherwise grow 30-fold and exp overflow fp32 (the tests assert the
    largest exponent): dash keeps its scale, diag = |x|^2 / 2 shrinks 900-fold, and the row norms of P grow."""
    H, D, M = ATTN_H, ATTN_D, ATTN_M
    rng = np.random.Generator(np.random.PCG64(seed))
    q, k, v = (rng.standard_normal((H, T, D)) * 0.3 * 10.0 ** rng.uniform(-1.0, 1.0, (H, T, D)) for _ in range(3))
    blocks = [np.linalg.qr(rng.standard_normal((D, D)))[0].T for _ in range(5)]
    P = np.concatenate(blocks)[:M] * np.linalg.norm(rng.standard_normal((M, D)), axis=1)[:, None] * pscale
    f = np.float32
    return (q / pscale).astype(f), (k / pscale).astype(f), v.astype(f), P.astype(f)
