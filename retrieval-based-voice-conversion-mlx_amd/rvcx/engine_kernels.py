"""Engine's wrappers of the kernel-level test entries (include/rvcx_test.h, _lib.TEST_SIG): single kernels, the planner
query and the comparison switches, for the numerics tests and the A/B tools. A mixin of rvcx.engine.Engine, which holds
the context, the plumbing (_check, _dev, stream) and the product methods.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _lib
from .config import SynthConfig


def _ptr(t) -> Optional[int]:
    return None if t is None else t.data_ptr()


class KernelTestMixin:
    # ------------------------------------------------------------------ comparison switches
    def set_dec_window(self, on: bool):
        """The generator's output window on (the default) or off (rvcx_set_dec_window, include/rvcx_test.h): with it
        on, the pipelines and stream groups run the generator only over the frames their trim keeps. Outputs are
        bit-identical either way."""
        self._check(self.lib.rvcx_set_dec_window(self.ctx, 1 if on else 0), "set_dec_window")

    def dec_margin_frames(self, cfg: SynthConfig = None) -> int:
        """The generator's one-sided receptive field in frames for `cfg` (default: the loaded configuration): the
        margin the output window keeps per cut side (rvcx_dec_margin_frames). Host only."""
        d = self._synth_desc(cfg if cfg is not None else self.synth_cfg)
        m = ctypes.c_int32(0)
        rc = self.lib.rvcx_dec_margin_frames(ctypes.byref(d), ctypes.byref(m))
        if rc != 0:
            raise _lib.RvcxError(rc, "dec_margin_frames: bad synthesizer configuration")
        return m.value

    def set_conv_math(self, mode: str):
        """Contraction arithmetic of this context: "h16" (the default: fp32 via three bf16 planes on bf16 MFMA, the
        generator's weight-streamed convs and fused ResBlock pairs via two fp16 planes), "split" (three bf16 planes
        everywhere) or "f32" (fp32-input MFMA) (rvcx_set_conv_math)."""
        m = {"default": 0, "f32": 1, "split": 2, "h16": 3}[mode]
        self._check(self.lib.rvcx_set_conv_math(self.ctx, m), "set_conv_math")
        self.conv_math = m

    # ------------------------------------------------------------------ FCPE's parts
    def fcpe_mel(self, audio):
        """The FCPE network's input alone (rvcx_fcpe_mel, include/rvcx_test.h): audio [N] -> log-mel [F, num_mels]."""
        self._need_fcpe()
        t = self.torch
        a = self._dev(audio, t.float32).reshape(-1)
        F = self._fcpe_frames(a.numel())
        mel = t.empty((F, self.fcpe_cfg["num_mels"]), dtype=t.float32, device=self.device)
        fo = ctypes.c_int64(0)
        self._check(self.lib.rvcx_fcpe_mel(self.ctx, a.data_ptr(), a.numel(), mel.data_ptr(), F, ctypes.byref(fo),
                                           self.stream()), "fcpe_mel")
        assert fo.value == F, (fo.value, F)
        return mel

    def performer_attention(self, q, k, v, proj):
        """The Performer attention kernels alone (rvcx_performer_attention, include/rvcx_test.h): q, k, v
        [H][T][64], proj [M][64] -> [H][T][64]."""
        t = self.torch
        q, k, v, pm = (self._dev(x, t.float32) for x in (q, k, v, proj))
        H, T, D = (int(x) for x in q.shape)
        if D != 64 or k.shape != q.shape or v.shape != q.shape or pm.shape[1] != 64:
            raise ValueError("performer_attention: q, k, v [H][T][64] and proj [M][64]")
        out = t.empty_like(q)
        self._check(self.lib.rvcx_performer_attention(self.ctx, q.data_ptr(), k.data_ptr(), v.data_ptr(), H, T,
                                                      pm.data_ptr(), int(pm.shape[0]), out.data_ptr(), self.stream()),
                    "performer_attention")
        return out

    def performer_attention_batch(self, q, k, v, proj):
        """rvcx_performer_attention_b (include/rvcx_test.h): q, k, v [B][H][T][64], proj [M][64] -> [B][H][T][64], the
        B streams in one set of launches."""
        t = self.torch
        q, k, v, pm = (self._dev(x, t.float32).contiguous() for x in (q, k, v, proj))
        if q.dim() != 4 or q.shape[3] != 64 or k.shape != q.shape or v.shape != q.shape or pm.shape[1] != 64:
            raise ValueError("performer_attention_batch: q, k, v [B][H][T][64] and proj [M][64]")
        B, H, T, _ = (int(x) for x in q.shape)
        out = t.empty_like(q)
        self._check(self.lib.rvcx_performer_attention_b(self.ctx, q.data_ptr(), k.data_ptr(), v.data_ptr(), B, H, T,
                                                        pm.data_ptr(), int(pm.shape[0]), out.data_ptr(),
                                                        self.stream()), "performer_attention_b")
        return out

    def performer_attention_v(self, q, k, v, T, proj):
        """performer_attention_batch for streams of different lengths in the same launches
        (rvcx_performer_attention_v): q, k, v [B][H][max(T)][64], T the B row counts -> [B][H][max(T)][64]; stream b's
        rows from T[b] on are neither read nor written (the output holds NaN there)."""
        t = self.torch
        q, k, v, pm = (self._dev(x, t.float32).contiguous() for x in (q, k, v, proj))
        if q.dim() != 4 or q.shape[3] != 64 or k.shape != q.shape or v.shape != q.shape or pm.shape[1] != 64:
            raise ValueError("performer_attention_v: q, k, v [B][H][T][64] and proj [M][64]")
        B, H, Tm, _ = (int(x) for x in q.shape)
        assert len(T) == B and max(T) == Tm
        Tv = (ctypes.c_int32 * B)(*[int(x) for x in T])
        out = t.full(q.shape, float("nan"), dtype=t.float32, device=self.device)
        self._check(self.lib.rvcx_performer_attention_v(self.ctx, q.data_ptr(), k.data_ptr(), v.data_ptr(), B, H, Tv, Tm,
                                                        pm.data_ptr(), int(pm.shape[0]), out.data_ptr(),
                                                        self.stream()), "performer_attention_v")
        return out

    # ------------------------------------------------------------------ streaming, index build, RMVPE and decoder parts
    def rt_model_rows(self, group, rows: int, gated: bool):
        """The model rows [rows, frames * upp] of a StreamGroup's last hop before (gated False) or after the noise
        gate (rvcx_rt_model_rows, include/rvcx_test.h); rows = that hop's active streams."""
        t = self.torch
        n = group.geometry["frames"] * self.upp
        out = t.empty((int(rows), n), dtype=t.float32, device=self.device)
        self._check(self.lib.rvcx_rt_model_rows(self.ctx, group.handle, 1 if gated else 0, out.data_ptr(), n,
                                                self.stream()), "rt_model_rows")
        return out

    def kmeans_assign(self, x, cent, want_dist: bool = True):
        """One nearest-centroid pass (rvcx_kmeans_assign): x [n, d], cent [nlist, d] -> (assign int32 [n],
        dist fp32 [n] or None) device tensors."""
        t = self.torch
        xx, cc = self._dev(x, t.float32), self._dev(cent, t.float32)
        n, d = xx.shape
        assign = t.empty((n,), dtype=t.int32, device=self.device)
        dist = t.empty((n,), dtype=t.float32, device=self.device) if want_dist else None
        self._check(self.lib.rvcx_kmeans_assign(self.ctx, xx.data_ptr(), n, d, cc.data_ptr(), cc.shape[0],
                                                assign.data_ptr(), _ptr(dist), self.stream()), "kmeans_assign")
        return assign, dist

    def kmeans_update(self, x, assign, cent):
        """One centroid update (rvcx_kmeans_update): -> (new centroids fp32 [nlist, d], sizes int64 [nlist])
        device tensors; cent is not modified."""
        t = self.torch
        xx, aa = self._dev(x, t.float32), self._dev(assign, t.int32)
        cc = self._dev(cent, t.float32).clone()
        n, d = xx.shape
        sizes = t.empty((cc.shape[0],), dtype=t.int64, device=self.device)
        self._check(self.lib.rvcx_kmeans_update(self.ctx, xx.data_ptr(), n, d, aa.data_ptr(), cc.shape[0],
                                                cc.data_ptr(), sizes.data_ptr(), self.stream()), "kmeans_update")
        return cc, sizes

    def gru_bidir(self, gi, whh_f, bhh_f, whh_b, bhh_b, tag_start: int = 0):
        """RMVPE's BiGRU recurrence alone (rvcx_gru_bidir, include/rvcx_test.h): gi [B, T, 1536], W_hh [768, 256] and
        b_hh [768] per direction -> out [B, T, 512] (device). tag_start < 0 continues the hand-off tag counters of the
        context's buffer, >= 0 zeroes the buffer and sets them."""
        t = self.torch
        g = self._dev(gi, t.float32)
        B, T, _ = g.shape
        assert g.shape[2] == 1536
        w = [self._dev(x, t.float32) for x in (whh_f, bhh_f, whh_b, bhh_b)]
        assert tuple(w[0].shape) == (768, 256) == tuple(w[2].shape) and w[1].numel() == 768 == w[3].numel()
        out = t.empty((B, T, 512), dtype=t.float32, device=self.device)
        self._check(self.lib.rvcx_gru_bidir(self.ctx, g.data_ptr(), B, T, w[0].data_ptr(), w[1].data_ptr(),
                                            w[2].data_ptr(), w[3].data_ptr(), out.data_ptr(), int(tag_start),
                                            self.stream()), "gru_bidir")
        return out

    def gru_bidir_v(self, gi, T, whh_f, bhh_f, whh_b, bhh_b, tag_start: int = 0):
        """gru_bidir for sequences of different lengths in the same launches (rvcx_gru_bidir_v): gi [B, max(T), 1536],
        T the B step counts -> out [B, max(T), 512] (device); sequence b's rows from T[b] on are not written (they hold
        NaN here)."""
        t = self.torch
        g = self._dev(gi, t.float32)
        B, Tm, _ = g.shape
        Tv = (ctypes.c_int32 * B)(*[int(v) for v in T])
        assert g.shape[2] == 1536 and len(T) == B and max(T) == Tm
        w = [self._dev(x, t.float32) for x in (whh_f, bhh_f, whh_b, bhh_b)]
        out = t.full((B, Tm, 512), float("nan"), dtype=t.float32, device=self.device)
        self._check(self.lib.rvcx_gru_bidir_v(self.ctx, g.data_ptr(), B, Tv, w[0].data_ptr(), w[1].data_ptr(),
                                              w[2].data_ptr(), w[3].data_ptr(), out.data_ptr(), int(tag_start),
                                              self.stream()), "gru_bidir_v")
        return out

    def dec_source(self, f0, eps_src=None, seed: int = 0):
        """The decoder's harmonic source alone (rvcx_dec_source, include/rvcx_test.h): f0 [B, T] -> har
        [B, T * upp] (device), NSF SineGen or the MRF source of the loaded configuration; eps_src as dec_only's."""
        t = self.torch
        f = self._dev(f0, t.float32)
        B, T = f.shape
        es = self._opt(eps_src, t.float32)
        out = t.empty((B, T * self.upp), dtype=t.float32, device=self.device)
        self._check(self.lib.rvcx_dec_source(self.ctx, B, T, f.data_ptr(), _ptr(es),
                                             self._seed(seed), out.data_ptr(), self.stream()),
                    "dec_source")
        return out

    # ------------------------------------------------------------------ RefineGAN's elementwise kernels
    def _f32_on_device(self, who, **tensors):
        t = self.torch
        for name, v in tensors.items():
            if v is not None and not (isinstance(v, t.Tensor) and v.dtype == t.float32 and v.device == self.device):
                raise ValueError(f"{who}: {name} must be a float32 tensor on {self.device}")

    def rg_resample_dw(self, x, ker, orig: int, width: int, y):
        """RefineGAN's kaiser-sinc downsampling kernel alone (rvcx_rg_resample_dw, include/rvcx_test.h): x
        [B][T_in][C], ker [2 width + orig] -> y [B][T_out][C], written in place. Every operand is a contiguous float32
        device tensor passed as it is (y may be a view into a larger guard buffer)."""
        self._f32_on_device("rg_resample_dw", x=x, ker=ker, y=y)
        B, T_in, C = (int(v) for v in x.shape)
        if not (x.is_contiguous() and y.is_contiguous() and ker.numel() == 2 * width + orig and
                tuple(y.shape[::2]) == (B, C)):
            raise ValueError("rg_resample_dw: x [B][T_in][C], ker [2 width + orig], y [B][T_out][C], contiguous")
        self._check(self.lib.rvcx_rg_resample_dw(self.ctx, x.data_ptr(), B, T_in, C, ker.data_ptr(), int(orig),
                                                 int(width), y.data_ptr(), int(y.shape[1]), self.stream()),
                    "rg_resample_dw")
        return y

    def rg_lerp_up_cat(self, x, C: int, rate: int, slope: float, skip, y):
        """RefineGAN's upsample + concat kernel alone (rvcx_rg_lerp_up_cat): x [B][T][ldx] (columns 0..C read), skip
        [B][T rate][Cd] -> y [B][T rate][ldy], columns 0..C + Cd written in place."""
        self._f32_on_device("rg_lerp_up_cat", x=x, skip=skip, y=y)
        B, T, ldx = (int(v) for v in x.shape)
        Cd, ldy = int(skip.shape[2]), int(y.shape[2])
        if not (x.is_contiguous() and skip.is_contiguous() and y.is_contiguous() and
                tuple(skip.shape[:2]) == (B, T * rate) == tuple(y.shape[:2])):
            raise ValueError("rg_lerp_up_cat: x [B][T][ldx], skip [B][T rate][Cd], y [B][T rate][ldy], contiguous")
        self._check(self.lib.rvcx_rg_lerp_up_cat(self.ctx, x.data_ptr(), B, T, int(C), ldx, int(rate), float(slope),
                                                 skip.data_ptr(), Cd, y.data_ptr(), ldy, self.stream()),
                    "rg_lerp_up_cat")
        return y

    def rg_adain(self, x, w, eps, y, slope: float = 0.2, mode: int = 0, div: float = 1.0, seed: int = 0):
        """RefineGAN's AdaIN kernel alone (rvcx_rg_adain): x, y [B][T][C], w [C], eps [B][C][T] or None (drawn from
        `seed`); mode 0 store, 1 add, 2 (y + v) / div, y written in place."""
        self._f32_on_device("rg_adain", x=x, w=w, eps=eps, y=y)
        B, T, C = (int(v) for v in x.shape)
        if not (x.is_contiguous() and y.is_contiguous() and tuple(y.shape) == (B, T, C) and w.numel() == C and
                (eps is None or (eps.is_contiguous() and tuple(eps.shape) == (B, C, T)))):
            raise ValueError("rg_adain: x, y [B][T][C], w [C], eps [B][C][T], contiguous")
        self._check(self.lib.rvcx_rg_adain(self.ctx, x.data_ptr(), B, T, C, w.data_ptr(), _ptr(eps),
                                           self._seed(seed), float(slope), y.data_ptr(),
                                           int(mode), float(div), self.stream()), "rg_adain")
        return y

    # ------------------------------------------------------------------ convs, attention, ResBlock pair
    def conv1d(self, x, w, bias=None, dilation: int = 1, padding: int = 0, stride: int = 1, math: str = "default"):
        """torch.nn.functional.conv1d(x.T[None], w, bias, stride, padding, dilation)[0].T on the device kernel:
        x [T][C_in] (time-major), w [N][C_in][taps] (torch layout) -> [T_out][N] fp32 (rvcx_conv1d)."""
        torch = self.torch
        x = self._dev(x, torch.float32)
        w = torch.as_tensor(w, dtype=torch.float32)
        N, C, K = (int(v) for v in w.shape)
        wk = self._dev(w.permute(2, 0, 1).contiguous(), torch.float32)
        b = self._dev(bias, torch.float32) if bias is not None else None
        T = int(x.shape[0])
        T_out = (T + 2 * padding - dilation * (K - 1) - 1) // stride + 1
        y = torch.empty((T_out, N), dtype=torch.float32, device=self.device)
        m = {"default": 0, "f32": 1, "split": 2, "wsb": 3, "gs": 4, "h16": 5, "f16": 6, "gs_h16": 7}[math]
        self._check(self.lib.rvcx_conv1d(self.ctx, _ptr(x), T, C, _ptr(wk), _ptr(b), N, K, dilation, padding, stride,
                                         m, _ptr(y), T_out, self.stream()), "conv1d")
        return y

    def conv1d_gen(self, x, w, bias=None, dilation: int = 1, padding: int = 0, pre_slope: float = 0.1,
                   slope=None, res=None, acc=None, acc_mode: int = 0, acc_div: float = 1.0,
                   kernel: str = "policy"):
        """The generator's fused conv (rvcx_conv1d_gen): y = acc(act(conv1d(pre(x), w, bias)) + res), pre = leaky
        ReLU(pre_slope) unless pre_slope is None, act = leaky ReLU(slope) unless slope is None, acc_mode 0 store / 1 add
        / 2 add-then-divide into `acc` (the
        initial y); kernel "policy", "wsb" (weight-streamed) or "wst" (weight-stationary). x [T][C_in], w [N][C_in][taps]
        -> [T_out][N] fp32 in the two-plane fp16 split."""
        torch = self.torch
        x = self._dev(x, torch.float32)
        w = torch.as_tensor(w, dtype=torch.float32)
        N, C, K = (int(v) for v in w.shape)
        wk = self._dev(w.permute(2, 0, 1).contiguous(), torch.float32)
        b = self._dev(bias, torch.float32) if bias is not None else None
        r = self._dev(res, torch.float32) if res is not None else None
        T = int(x.shape[0])
        T_out = T + 2 * padding - dilation * (K - 1)
        if acc is not None:
            y = self._dev(acc, torch.float32).clone()
        else:
            y = torch.empty((T_out, N), dtype=torch.float32, device=self.device)
        kn = {"policy": 0, "wsb": 1, "wst": 2}[kernel]
        self._check(self.lib.rvcx_conv1d_gen(self.ctx, _ptr(x), T, C, _ptr(wk), _ptr(b), N, K, dilation, padding,
                                             0 if pre_slope is None else 1,
                                             0.0 if pre_slope is None else float(pre_slope), 0 if slope is None else 1,
                                             0.0 if slope is None else float(slope), _ptr(r), int(acc_mode),
                                             float(acc_div), kn, _ptr(y), self.stream()), "conv1d_gen")
        return y

    ROUTES = {"policy": 0, "f32": 1, "emu": 2, "wsb": 3, "gs": 4, "wst": 5}

    def conv1d_ex(self, x, w, y, *, T_in: int, C_in: int, N: int, T_out: int, ldx: int, ldy: int, taps: int = 1,
                  dil: int = 1, pad: int = 0, stride: int = 1, ldr: int = 0, bias=None, res=None, mask=None,
                  pre_mask=None, batch: int = 1, x_bs: int = 0, y_bs: int = 0, res_bs: int = 0, mask_bs: int = 0,
                  pre_mask_bs: int = 0, batch_inner: int = 1, x_bs2: int = 0, w_bs2: int = 0, y_bs2: int = 0,
                  res_bs2: int = 0, bias_bs2: int = 0, pre_act: int = 0, pre_slope: float = 0.0, act: int = 0,
                  slope: float = 0.0, alpha: float = 1.0, res_mode: int = 0, acc_mode: int = 0, acc_div: float = 1.0,
                  gate_h: int = 0, gate_g=None, gate_g_bs: int = 0, ln_g=None, ln_b=None, ln_eps: float = 1e-5,
                  nz_har=None, nz_bs: int = 0, nz_stride: int = 0, nz_kk: int = 0, nz_u: int = 1, nz_C: int = 0,
                  nz_w=None, nz_b=None, route="policy", no_splitk: bool = False):
        """One 1-D contraction in any form the runtime issues (rvcx_conv1d_ex, include/rvcx_test.h): the fields of the
        dispatcher's record, strides in floats. Every operand is a float32 tensor on this device and is passed as it
        is -- a view's offset is its base pointer, nothing is copied or made contiguous -- and `y` is written in place.
        Each operand's extent (the last element the form addresses) is checked against the storage behind its tensor
        before the launch (ValueError). Returns (y, kernel family name, planned split count)."""
        torch = self.torch
        G, B, i64 = int(batch_inner), int(batch), int

        def span(t, name, last):
            """`last`: the largest element offset from t's first element that the form addresses."""
            if t is None:
                return None
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == self.device):
                raise ValueError(f"conv1d_ex: {name} must be a float32 tensor on {self.device}")
            room = t.untyped_storage().nbytes() // 4 - t.storage_offset()
            if last < 0 or last >= room:
                raise ValueError(f"conv1d_ex: {name} addresses element {last}, its storage holds {room} from the view")
            return t.data_ptr()

        ncol = gate_h if gate_h > 0 else N
        d = _lib.ConvTestDesc()
        d.x = span(x, "x", (B - 1) * x_bs + (G - 1) * x_bs2 + (T_in - 1) * ldx + C_in - 1)
        d.w = span(w, "w", (G - 1) * w_bs2 + taps * N * C_in - 1)
        d.y = span(y, "y", (B - 1) * y_bs + (G - 1) * y_bs2 + (T_out - 1) * ldy + ncol - 1)
        d.bias = span(bias, "bias", (G - 1) * bias_bs2 + N - 1)
        d.res = span(res, "res", (B - 1) * res_bs + (G - 1) * res_bs2 + (T_out - 1) * ldr + N - 1)
        d.mask = span(mask, "mask", (B - 1) * mask_bs + T_out - 1)
        d.pre_mask = span(pre_mask, "pre_mask", (B - 1) * pre_mask_bs + T_in - 1)
        d.gate_g = span(gate_g, "gate_g", (B - 1) * gate_g_bs + N - 1)
        d.ln_g, d.ln_b = span(ln_g, "ln_g", N - 1), span(ln_b, "ln_b", N - 1)
        d.nz_har = span(nz_har, "nz_har", (B - 1) * nz_bs + (T_out * nz_u - 1) * nz_stride + max(nz_kk, 1) - 1)
        d.nz_w = span(nz_w, "nz_w", nz_C * max(nz_stride, 1) * max(-(-nz_kk // max(nz_stride, 1)), 1) - 1)
        d.nz_b = span(nz_b, "nz_b", nz_C - 1)
        for k, v in dict(T_in=T_in, C_in=C_in, N=N, taps=taps, dil=dil, pad=pad, stride=stride, T_out=T_out, ldx=ldx,
                         ldy=ldy, ldr=ldr, batch=B, x_bs=x_bs, y_bs=y_bs, res_bs=res_bs, mask_bs=mask_bs,
                         pre_mask_bs=pre_mask_bs, batch_inner=G, x_bs2=x_bs2, w_bs2=w_bs2, y_bs2=y_bs2,
                         res_bs2=res_bs2, bias_bs2=bias_bs2, pre_act=pre_act, act=act, res_mode=res_mode,
                         acc_mode=acc_mode, gate_h=gate_h, gate_g_bs=gate_g_bs, nz_bs=nz_bs, nz_stride=nz_stride,
                         nz_kk=nz_kk, nz_u=nz_u, nz_C=nz_C).items():
            setattr(d, k, i64(v))
        d.pre_slope, d.slope, d.alpha, d.acc_div, d.ln_eps = (float(pre_slope), float(slope), float(alpha),
                                                              float(acc_div), float(ln_eps))
        d.route = self.ROUTES[route] if isinstance(route, str) else int(route)
        d.no_splitk = 1 if no_splitk else 0
        self.last_conv_desc = d  # what conv_plan() queries the planner with
        kind, ksplit = ctypes.c_int(-1), ctypes.c_int(0)
        self._check(self.lib.rvcx_conv1d_ex(self.ctx, ctypes.byref(d), ctypes.byref(kind), ctypes.byref(ksplit),
                                            self.stream()), "conv1d_ex")
        name = self.lib.rvcx_profile_kind_name(kind.value)
        return y, (name.decode() if name else "other"), int(ksplit.value)

    def conv_plan(self, desc=None, static_weight: bool = True):
        """What the planner decides under the size policy for a conv1d_ex descriptor (the last one launched unless given)
        in this context's arithmetic: (kernel family name, tile id, split count, weight image format). Host only
        (rvcx_conv_plan, include/rvcx_test.h)."""
        out = [ctypes.c_int(-1) for _ in range(4)]
        d = self.last_conv_desc if desc is None else desc
        self._check(self.lib.rvcx_conv_plan(ctypes.byref(d), None, 0, 1 if static_weight else 0,
                                            getattr(self, "conv_math", 0), 0, -1, -1, *[ctypes.byref(o) for o in out]),
                    "conv_plan")
        name = self.lib.rvcx_profile_kind_name(out[0].value)
        return (name.decode() if name else "other"), out[1].value, out[2].value, out[3].value

    def conv2d3x3(self, x, w, bias=None, relu: bool = False, math: str = "default"):
        """torch.nn.functional.conv2d(x.permute(2, 0, 1)[None], w, bias, padding=1)[0].permute(1, 2, 0) on the device
        kernel: x [H][W][C_in] (NHWC), w [N][C_in][3][3] (torch layout) -> [H][W][N] fp32 (rvcx_conv2d3x3); math
        "default" = the context's arithmetic, "f32" = exact fp32, "gsw" = the U-Net deep levels' windowed kernel in the
        fp16 split (K split over workgroups)."""
        torch = self.torch
        x = self._dev(x, torch.float32)
        w = torch.as_tensor(w, dtype=torch.float32)
        N, C = int(w.shape[0]), int(w.shape[1])
        wk = self._dev(w.permute(2, 3, 0, 1).reshape(9, N, C).contiguous(), torch.float32)
        b = self._dev(bias, torch.float32) if bias is not None else None
        H, W = int(x.shape[0]), int(x.shape[1])
        y = torch.empty((H, W, N), dtype=torch.float32, device=self.device)
        m = {"default": 0, "f32": 1, "gsw": 2}[math]
        self._check(self.lib.rvcx_conv2d3x3(self.ctx, _ptr(x), H, W, C, _ptr(wk), _ptr(b), N, 1 if relu else 0, m,
                                            _ptr(y), self.stream()), "conv2d3x3")
        return y

    def convtranspose2d_s2(self, x, w, bias=None, relu: bool = False, math: str = "default"):
        """torch.nn.functional.conv_transpose2d(x.permute(2, 0, 1)[None], w, bias, stride=2, padding=1,
        output_padding=1)[0].permute(1, 2, 0) on the device (rvcx_convtranspose2d_s2, the U-Net decoder's up-conv as
        the pipeline runs it): x [H][W][C_in] (NHWC), w [C_in][N][3][3] (torch layout) -> [2H][2W][N] fp32; math
        "default" = the context's arithmetic, "f32" = exact fp32."""
        torch = self.torch
        x = self._dev(x, torch.float32)
        wd = self._dev(torch.as_tensor(w, dtype=torch.float32).contiguous(), torch.float32)
        C, N = int(wd.shape[0]), int(wd.shape[1])
        b = self._dev(bias, torch.float32) if bias is not None else None
        H, W = int(x.shape[0]), int(x.shape[1])
        y = torch.empty((2 * H, 2 * W, N), dtype=torch.float32, device=self.device)
        m = {"default": 0, "f32": 1}[math]
        self._check(self.lib.rvcx_convtranspose2d_s2(self.ctx, _ptr(x), H, W, C, _ptr(wd), _ptr(b), N,
                                                     1 if relu else 0, m, _ptr(y), self.stream()), "convtranspose2d_s2")
        return y

    def conv2d3x3_v(self, x, heights, w, bias=None, relu: bool = False, math: str = "default"):
        """conv2d3x3 on B images of different heights in one launch (rvcx_conv2d3x3_v): x [B][H_max][W][C_in], heights
        the B own heights -> [B][H_max][W][N]; image b's rows below heights[b] are conv2d3x3's on x[b, :heights[b]], a
        tap from row heights[b] on reading zero whatever x holds there."""
        torch = self.torch
        x = self._dev(x, torch.float32).contiguous()
        w = torch.as_tensor(w, dtype=torch.float32)
        N, C = int(w.shape[0]), int(w.shape[1])
        wk = self._dev(w.permute(2, 3, 0, 1).reshape(9, N, C).contiguous(), torch.float32)
        b = self._dev(bias, torch.float32) if bias is not None else None
        B, H, W = (int(v) for v in x.shape[:3])
        hv = (ctypes.c_int32 * B)(*[int(v) for v in heights])
        y = torch.empty((B, H, W, N), dtype=torch.float32, device=self.device)
        m = {"default": 0, "f32": 1, "gsw": 2}[math]
        self._check(self.lib.rvcx_conv2d3x3_v(self.ctx, _ptr(x), B, hv, H, W, C, _ptr(wk), _ptr(b), N,
                                              1 if relu else 0, m, _ptr(y), self.stream()), "conv2d3x3_v")
        return y

    def convtranspose2d_s2_v(self, x, heights, w, bias=None, relu: bool = False, math: str = "default"):
        """convtranspose2d_s2 on B images of different heights in one launch (rvcx_convtranspose2d_s2_v): x
        [B][H_max][W][C_in] -> [B][2 H_max][2 W][N]; image b's rows below 2 heights[b] are convtranspose2d_s2's on
        x[b, :heights[b]]."""
        torch = self.torch
        x = self._dev(x, torch.float32).contiguous()
        wd = self._dev(torch.as_tensor(w, dtype=torch.float32).contiguous(), torch.float32)
        C, N = int(wd.shape[0]), int(wd.shape[1])
        b = self._dev(bias, torch.float32) if bias is not None else None
        B, H, W = (int(v) for v in x.shape[:3])
        hv = (ctypes.c_int32 * B)(*[int(v) for v in heights])
        y = torch.empty((B, 2 * H, 2 * W, N), dtype=torch.float32, device=self.device)
        m = {"default": 0, "f32": 1}[math]
        self._check(self.lib.rvcx_convtranspose2d_s2_v(self.ctx, _ptr(x), B, hv, H, W, C, _ptr(wd), _ptr(b), N,
                                                       1 if relu else 0, m, _ptr(y), self.stream()),
                    "convtranspose2d_s2_v")
        return y

    def flash_attention(self, qkv, n_heads: int, qscale: float, rel_k=None, rel_v=None, window: int = 0, mask=None):
        """The fused attention core (rvcx_flash_attention): qkv [B][T][3 H] time-major (q | k | v, heads of dk inside
        each), optional relative tables rel_k / rel_v [2 window + 1][dk] and key/query mask [B][T] -> [B][T][H]."""
        torch = self.torch
        q = self._dev(qkv, torch.float32)
        B, T, H3 = (int(v) for v in q.shape)
        dk = H3 // 3 // n_heads
        rk = self._opt(rel_k, torch.float32)
        rv = self._opt(rel_v, torch.float32)
        mk = self._opt(mask, torch.float32)
        y = torch.empty((B, T, H3 // 3), dtype=torch.float32, device=self.device)
        self._check(self.lib.rvcx_flash_attention(self.ctx, _ptr(q), B, T, int(n_heads), dk, float(qscale), _ptr(rk),
                                                  _ptr(rv), int(window), _ptr(mk), _ptr(y), self.stream()),
                    "flash_attention")
        return y

    def resblock_pair(self, x, w1, b1, w2, b2, dilation: int, acc=None, acc_mode: int = 0, acc_div: float = 1.0,
                      cfg: int = 0):
        """One ResBlock dilation pair on the fused kernel (rvcx_resblock_pair): x [B][T][C] time-major, w1/w2
        [C][C][k] (torch layout) -> conv2(lrelu(conv1_d(lrelu(x)) + b1)) + b2 + x, stored (acc_mode 0) or
        accumulated into `acc` (1: acc + out, 2: (acc + out) / acc_div)."""
        torch = self.torch
        x = self._dev(x, torch.float32)
        B, T, C = (int(v) for v in x.shape)
        k = int(np.shape(w1)[2])
        w1k = self._dev(torch.as_tensor(w1, dtype=torch.float32).permute(2, 0, 1).contiguous(), torch.float32)
        w2k = self._dev(torch.as_tensor(w2, dtype=torch.float32).permute(2, 0, 1).contiguous(), torch.float32)
        b1d, b2d = self._dev(b1, torch.float32), self._dev(b2, torch.float32)
        y = (self._dev(acc, torch.float32).clone() if acc is not None
             else torch.empty((B, T, C), dtype=torch.float32, device=self.device))
        self._check(self.lib.rvcx_resblock_pair(self.ctx, _ptr(x), B, T, C, _ptr(w1k), _ptr(b1d), _ptr(w2k), _ptr(b2d),
                                                k, dilation, acc_mode, float(acc_div), cfg, _ptr(y), self.stream()),
                    "resblock_pair")
        return y
