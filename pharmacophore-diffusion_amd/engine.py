"""PfEngine: one libpfdyn handle per (process, GPU).  Marshals torch tensors (device memory owned
by PyTorch) and the current torch HIP stream into the C ABI of include/pfdyn.h."""
import contextlib
import ctypes
from typing import Dict, Optional

import torch

from . import _lib as L


def _stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dptr(t: Optional[torch.Tensor]):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device tensors must be contiguous CUDA/HIP tensors"
    return ctypes.c_void_p(t.data_ptr())


def _i32_host(t: torch.Tensor):
    """contiguous int32 numpy copy of an index tensor (host)."""
    import numpy as np
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.int32)


def _f32(t: torch.Tensor, device) -> torch.Tensor:
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


class PfEngine:
    def __init__(self, *, pharm_nf=6, rec_nf=11, vector_size=16, n_hidden_scalars=128, n_convs=2,
                 n_message_gvps=3, n_update_gvps=2, n_noise_gvps=4, message_norm="mean", ff_k=0, pf_k=5,
                 graph_cutoffs=None, rbf_dmax=15.0, rbf_dim=16, device=None):
        self.lib = L.load()
        if not torch.cuda.is_available():
            raise L.PfError("no HIP device visible to PyTorch: libpfdyn has no CPU fallback")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        cut = {"pp": 3.5, "pf": 8.0, "fp": 8.0, "ff": 9.0}
        cut.update(graph_cutoffs or {})
        if isinstance(message_norm, dict):
            raise L.PfError("dict-valued message_norm is unusable in the reference too (gvp.py:453)")
        if message_norm == "mean":
            mode, val = L.PF_NORM_MEAN, 1.0
        elif float(message_norm) == 0.0:
            mode, val = L.PF_NORM_GRAPH, 0.0
        else:
            mode, val = L.PF_NORM_VALUE, float(message_norm)
        self.cfg = L.PfConfig(L.PF_ABI_VERSION, pharm_nf, rec_nf, vector_size, n_hidden_scalars, n_convs,
                              n_message_gvps, n_update_gvps, n_noise_gvps, mode, val, int(ff_k), int(pf_k),
                              float(cut["pp"]), float(cut["pf"]), float(cut["fp"]), float(cut["ff"]),
                              float(rbf_dmax), int(rbf_dim))
        self.pharm_nf, self.rec_nf = pharm_nf, rec_nf
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.lib.pf_create(ctypes.byref(self.cfg), ctypes.byref(self._h))
        if rc < 0:
            msg = self.lib.pf_last_error(None)
            raise L.PfError(f"pf_create failed ({rc}): {msg.decode() if msg else ''}")
        self.Nf = self.Np = self.B = 0
        self._keep = []

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                self.lib.pf_destroy(self._h)
                self._h = ctypes.c_void_p()
        except Exception:
            pass

    def _ck(self, rc, what):
        return L.check(self.lib, self._h, rc, what)

    # -- weights (reference state_dict key layout) -------------------------------------------
    def load_state_dict(self, sd: Dict[str, torch.Tensor], prefix: str = "dynamics."):
        """sd: reference keys (``dynamics.*``); ``prefix`` is what the given keys start with
        relative to the reference layout (pass prefix='' for a bare PharmRecDynamicsGVP dict)."""
        with torch.cuda.device(self.device):
            for k, v in sd.items():
                name = k if prefix == "dynamics." else "dynamics." + k
                if not name.startswith("dynamics."):
                    continue           # e.g. gamma.gamma
                t = v.detach().to("cpu", torch.float32).contiguous()
                shape = (ctypes.c_int64 * max(t.dim(), 1))(*t.shape)
                self._ck(self.lib.pf_set_weight(self._h, name.encode(), ctypes.c_void_p(t.data_ptr()) if t.numel() else None,
                                                t.dim(), shape), f"pf_set_weight({name})")
            self._ck(self.lib.pf_commit_weights(self._h), "pf_commit_weights")

    # -- static batch --------------------------------------------------------------------------
    def _upload(self, t: torch.Tensor) -> torch.Tensor:
        """fp32 device copy of a host tensor through pinned memory (a pageable host -> device copy waits for everything
        already enqueued on the stream, i.e. for the previous batch); device tensors pass through."""
        if t.is_cuda:
            return _f32(t, self.device)
        return t.detach().to(torch.float32).contiguous().pin_memory().to(self.device, non_blocking=True)

    def set_batch(self, prot_x, prot_h, prot_ptr, pharm_ptr, pp_src, pp_dst, pocket_uid=None):
        """pf_set_pocket_batch / pf_set_pocket_batch_host: asynchronous on the current stream.  ``pocket_uid`` ([B]
        integers, optional): graphs with equal values are claimed to be copies of one pocket (PocketGraph.pocket_uid), which
        lets them share conv layer 0's protein-protein messages during sampling.  The claim is verified before it is used:
        the library checks atom counts, pp in-degrees and pp sources of every copy, and coordinates and features byte for
        byte when the pocket tensors are host-resident; for device-resident tensors (which the library never reads on the
        host) the coordinate / feature comparison is done here, on the device.  A false claim raises PfError."""
        import numpy as np
        # index arrays: int32 host copies through numpy (single-threaded; a torch dtype conversion of half a million
        # elements goes through the intra-op thread pool, whose wake-up stalls for tens of milliseconds now and then on
        # hosts with hundreds of hardware threads)
        pptr, fptr, src, dst = (_i32_host(t) for t in (prot_ptr, pharm_ptr, pp_src, pp_dst))
        on_host = not prot_x.is_cuda and not prot_h.is_cuda
        rep = None
        if pocket_uid is not None:
            uid = np.asarray(pocket_uid.detach().cpu().numpy() if isinstance(pocket_uid, torch.Tensor) else pocket_uid).reshape(-1)
            first = {}
            rep = np.asarray([first.setdefault(int(u), i) for i, u in enumerate(uid)], dtype=np.int32)
            if len(first) == rep.size:
                rep = None                                # no pocket has copies
        if rep is not None and not on_host and rep.size == pptr.size - 1:
            cnt = np.diff(pptr)
            if np.array_equal(cnt, cnt[rep]):             # (unequal atom counts: the library refuses the claim itself)
                # atom i of a copy <-> the same atom of its representative: one gather and one comparison on the device
                idx = np.concatenate([np.arange(pptr[r], pptr[r + 1]) for r in rep]) if rep.size else np.zeros(0, np.int64)
                idx_t = torch.from_numpy(idx.astype(np.int64)).to(prot_x.device)
                same = bool(torch.equal(prot_x, prot_x[idx_t])) and bool(torch.equal(prot_h.to(prot_x.device), prot_h.to(prot_x.device)[idx_t]))
                if not same:
                    raise L.PfError("pf_set_pocket_groups: a graph is not a copy of the pocket it names (coordinates / features differ)")
        # the claim always travels with its bind (an empty one clears whatever an earlier, failed bind left behind)
        if rep is not None:
            self._ck(self.lib.pf_set_pocket_groups(self._h, int(rep.size), rep.ctypes.data), "pf_set_pocket_groups")
        else:
            self._ck(self.lib.pf_set_pocket_groups(self._h, 0, None), "pf_set_pocket_groups")
        self.B = int(pptr.size - 1)
        self.Np, self.Nf = int(pptr[-1]), int(fptr[-1])
        with torch.cuda.device(self.device):
            args = (int(src.size), src.ctypes.data if src.size else None, dst.ctypes.data if dst.size else None, _stream_ptr())
            if on_host:
                # host-resident pockets (the sampling drivers): the library stages them with its tables -- one upload, the
                # one-hot check on the host copy, nothing waits for the device
                hx = np.ascontiguousarray(prot_x.detach().numpy(), dtype=np.float32)
                hh = np.ascontiguousarray(prot_h.detach().numpy(), dtype=np.float32)
                self._ck(self.lib.pf_set_pocket_batch_host(self._h, self.B, pptr.ctypes.data, fptr.ctypes.data, hx.ctypes.data,
                                                           hh.ctypes.data, *args), "pf_set_pocket_batch_host")
            else:
                px, ph = self._upload(prot_x), self._upload(prot_h)
                self._ck(self.lib.pf_set_pocket_batch(self._h, self.B, pptr.ctypes.data, fptr.ctypes.data, _dptr(px), _dptr(ph),
                                                      *args), "pf_set_pocket_batch")

    def build_pp_edges(self, prot_x, prot_ptr, max_num_neighbors=100):
        px = _f32(prot_x, self.device)
        pptr = prot_ptr.to("cpu", torch.int32).contiguous()
        B = int(pptr.numel() - 1)
        with torch.cuda.device(self.device):
            n = self._ck(self.lib.pf_build_pp_edges(self._h, B, pptr.data_ptr(), _dptr(px), max_num_neighbors,
                                                    None, None, 0, _stream_ptr()), "pf_build_pp_edges")
            src = torch.zeros(max(n, 1), dtype=torch.int32)
            dst = torch.zeros(max(n, 1), dtype=torch.int32)
            self._ck(self.lib.pf_build_pp_edges(self._h, B, pptr.data_ptr(), _dptr(px), max_num_neighbors,
                                                src.data_ptr(), dst.data_ptr(), n, _stream_ptr()), "pf_build_pp_edges")
        return src[:n].long(), dst[:n].long()

    # -- the boundary function -----------------------------------------------------------------
    def dynamics(self, pharm_x, pharm_h, t, prot_x=None):
        x, hh, tt = _f32(pharm_x, self.device), _f32(pharm_h, self.device), _f32(t, self.device)
        px = _f32(prot_x, self.device) if prot_x is not None else None
        eps_h = torch.empty(self.Nf, self.pharm_nf, device=self.device)
        eps_x = torch.empty(self.Nf, 3, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_dynamics_forward(self._h, _dptr(px), _dptr(x), _dptr(hh), _dptr(tt), _dptr(eps_h),
                                                  _dptr(eps_x), _stream_ptr()), "pf_dynamics_forward")
        return eps_h, eps_x

    # -- training step (gradients of the boundary function) -------------------------------------
    def param_layout(self):
        """[(reference key, offset, numel)] of the flat parameter / gradient vector (state-dict order)."""
        n = ctypes.c_int64()
        nt = ctypes.c_int32()
        self._ck(self.lib.pf_param_count(self._h, ctypes.byref(n), ctypes.byref(nt)), "pf_param_count")
        out = []
        for i in range(nt.value):
            name = ctypes.c_char_p()
            off = ctypes.c_int64()
            cnt = ctypes.c_int64()
            self._ck(self.lib.pf_param_layout(self._h, i, ctypes.byref(name), ctypes.byref(off), ctypes.byref(cnt)), "pf_param_layout")
            out.append((name.value.decode(), off.value, cnt.value))
        self.n_params = n.value
        return out

    def train_forward(self, pharm_x, pharm_h, t, prot_x=None, dropout=0.0, seed=0):
        """PharmRecDynamicsGVP.forward in train() mode; keeps the per-layer state for train_backward."""
        x, hh, tt = _f32(pharm_x, self.device), _f32(pharm_h, self.device), _f32(t, self.device)
        px = _f32(prot_x, self.device) if prot_x is not None else None
        eps_h = torch.empty(self.Nf, self.pharm_nf, device=self.device)
        eps_x = torch.empty(self.Nf, 3, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_train_forward(self._h, _dptr(px), _dptr(x), _dptr(hh), _dptr(tt), float(dropout),
                                               int(seed) & 0xFFFFFFFF, _dptr(eps_h), _dptr(eps_x), _stream_ptr()),
                     "pf_train_forward")
        return eps_h, eps_x

    def train_backward(self, g_eps_h, g_eps_x, input_grads=False):
        """d(loss)/d(parameters) as one flat vector (see param_layout) given d(loss)/d(eps).  input_grads: also the gradient
        w.r.t. the inputs of the last train_forward -- returns (grad, g_x_t [Nf, 3], g_h_t [Nf, pharm_nf]); True asks for both,
        a pair of flags (x_t, h_t) for either (the other comes back as None).  On the wide training family, or on the tuned one
        (fp32) with set_train_input_grads(True)."""
        gh, gx = _f32(g_eps_h, self.device), _f32(g_eps_x, self.device)
        if not hasattr(self, "n_params"):
            self.param_layout()
        grad = torch.empty(self.n_params, device=self.device)
        if input_grads is False:
            with torch.cuda.device(self.device):
                self._ck(self.lib.pf_train_backward(self._h, _dptr(gh), _dptr(gx), _dptr(grad), _stream_ptr()), "pf_train_backward")
            return grad
        want_x, want_h = (True, True) if input_grads is True else (bool(input_grads[0]), bool(input_grads[1]))
        g_x_t = torch.empty(self.Nf, 3, device=self.device) if want_x else None
        g_h_t = torch.empty(self.Nf, self.pharm_nf, device=self.device) if want_h else None
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_train_backward_inputs(self._h, _dptr(gh), _dptr(gx), _dptr(grad), _dptr(g_x_t), _dptr(g_h_t),
                                                       _stream_ptr()), "pf_train_backward_inputs")
        return grad, g_x_t, g_h_t

    def input_vjp(self, g_eps_h, g_eps_x, want=(True, True)):
        """The gradients of sum(eps_h * g_eps_h) + sum(eps_x * g_eps_x) w.r.t. the inputs of the last train_forward ALONE
        (pf_dynamics_input_vjp): (g_x_t [Nf, 3], g_h_t [Nf, pharm_nf]), None where ``want`` says no.  No parameter gradient is
        formed; the bits are those of train_backward(..., input_grads=...).  On the wide training family, or on the tuned one
        (fp32) with set_train_input_grads(True)."""
        gh, gx = _f32(g_eps_h, self.device), _f32(g_eps_x, self.device)
        g_x_t = torch.empty(self.Nf, 3, device=self.device) if want[0] else None
        g_h_t = torch.empty(self.Nf, self.pharm_nf, device=self.device) if want[1] else None
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_dynamics_input_vjp(self._h, _dptr(gh), _dptr(gx), _dptr(g_x_t), _dptr(g_h_t), _stream_ptr()),
                     "pf_dynamics_input_vjp")
        return g_x_t, g_h_t

    def train_loss_forward(self, pharm_x0, pharm_h0, t_int, eps_x, eps_h, alpha_tab, sigma_tab, n_timesteps, feat_norm,
                           remove_com=True, weighted_loss=False, dropout=0.0, seed=0, ep_coord=False, ep_feat=False):
        """PharmacophoreDiff.forward (pharmacodiff.py:162-243) around the bound batch as one call: COM removal, noising, the
        train-mode dynamics, losses and metrics.  ep_coord / ep_feat: the reference's endpoint_param_coord / endpoint_param_feat
        (the dynamics predict the clean coordinates / the type logits instead of the noise).  Returns a device tensor [9]:
        pos loss, feat loss, position error, weighted position error, accuracy, weighted accuracy, then what a step derives
        from them -- total loss, total error, weighted total error."""
        x0, h0 = _f32(pharm_x0, self.device), _f32(pharm_h0, self.device)
        ex, eh = _f32(eps_x, self.device), _f32(eps_h, self.device)
        ti = t_int.to(self.device, torch.int32).contiguous()
        al, sg = _f32(alpha_tab, self.device), _f32(sigma_tab, self.device)
        out = torch.empty(9, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_train_loss_forward_ep(self._h, _dptr(x0), _dptr(h0), _dptr(ti), _dptr(ex), _dptr(eh), _dptr(al),
                                                       _dptr(sg), int(n_timesteps), float(feat_norm), int(bool(remove_com)),
                                                       int(bool(weighted_loss)), int(bool(ep_coord)), int(bool(ep_feat)),
                                                       float(dropout), int(seed) & 0xFFFFFFFF, _dptr(out), _stream_ptr()),
                     "pf_train_loss_forward_ep")
        return out

    def _grad_out(self, out):
        if not hasattr(self, "n_params"):
            self.param_layout()
        if out is None:
            return torch.empty(self.n_params, device=self.device)
        if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != self.n_params or out.device != self.device:
            raise ValueError("`out` must be a contiguous fp32 vector of n_params elements on the engine's device")
        return out

    def train_loss_backward(self, g_pos, g_feat, out=None):
        """d(g_pos * pos loss + g_feat * feat loss)/d(parameters) of the last train_loss_forward, as one flat vector.
        out: an existing flat fp32 device vector to receive the gradient (every element is stored, nothing is accumulated)."""
        gp, gf = _f32(g_pos, self.device).reshape(1), _f32(g_feat, self.device).reshape(1)
        grad = self._grad_out(out)
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_train_loss_backward(self._h, _dptr(gp), _dptr(gf), _dptr(grad), _stream_ptr()),
                     "pf_train_loss_backward")
        return grad

    def train_loss_backward_out(self, g_out, out=None):
        """The same from the upstream gradient of train_loss_forward's whole output vector ([9]; entries 0, 1 and 6 count).
        out: an existing flat fp32 device vector to receive the gradient (every element is stored, nothing is accumulated)."""
        go = _f32(g_out, self.device).reshape(9)
        grad = self._grad_out(out)
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_train_loss_backward_out(self._h, _dptr(go), _dptr(grad), _stream_ptr()),
                     "pf_train_loss_backward_out")
        return grad

    def set_flat_params(self, flat):
        """Replace every parameter from one flat device vector (param_layout order); the packed kernel weights are
        refreshed by a device-side gather."""
        f = _f32(flat, self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_set_flat_params(self._h, _dptr(f), _stream_ptr()), "pf_set_flat_params")

    def get_flat_params(self):
        if not hasattr(self, "n_params"):
            self.param_layout()
        out = torch.empty(self.n_params, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_get_flat_params(self._h, _dptr(out), _stream_ptr()), "pf_get_flat_params")
        return out

    def adam_step(self, params, grad, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        """Fused Adam on flat device vectors (in place) + refresh of the engine's weights from ``params``."""
        for t in (params, grad, exp_avg, exp_avg_sq):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == self.n_params
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_adam_step(self._h, _dptr(params), _dptr(grad), _dptr(exp_avg), _dptr(exp_avg_sq), int(step),
                                           float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                           _stream_ptr()), "pf_adam_step")

    # -- the guarded optimiser step (pf_adam_step_guarded): clipping, non-finite skip, EMA, grad_scale -------------------
    def optim_state(self, applied_steps=0):
        """A fresh state block of the guarded step (PF_OPTIM_STATE_BYTES on the device, pf_optim_state_init): applied_steps is 0
        for a new run, the checkpoint's count on a resume."""
        state = torch.empty(L.PF_OPTIM_STATE_BYTES // 8, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_optim_state_init(self._h, _dptr(state), int(applied_steps), _stream_ptr()), "pf_optim_state_init")
        return state

    @staticmethod
    def read_optim_state(state):
        """The state block as a dict (applied, skipped, norm, coef, finite).  Copies it to the host: SYNCHRONISES."""
        raw = state.cpu().numpy().tobytes()
        import struct
        applied, skipped, norm, coef, finite = struct.unpack_from("<qqffi", raw, 0)
        return {"applied": applied, "skipped": skipped, "norm": norm, "coef": coef, "finite": bool(finite)}

    @staticmethod
    def _optim_opts(lr, betas, eps, weight_decay, grad_scale, clip_norm, clip_value, ema_decay):
        if clip_norm is not None and clip_value is not None:
            raise ValueError("clip_norm and clip_value are mutually exclusive")
        mode, clip = ((L.PF_CLIP_NORM, clip_norm) if clip_norm is not None else
                      (L.PF_CLIP_VALUE, clip_value) if clip_value is not None else (L.PF_CLIP_NONE, 0.0))
        return L.PfOptimOpts(float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), float(grad_scale),
                             int(mode), float(clip), float(ema_decay or 0.0))

    def _optim_vectors(self, n, params, grad, exp_avg, exp_avg_sq, ema, state):
        for t in (params, grad, exp_avg, exp_avg_sq) + ((ema,) if ema is not None else ()):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n
        assert state.is_cuda and state.dtype == torch.int64 and state.numel() * 8 == L.PF_OPTIM_STATE_BYTES

    def adam_step_guarded(self, params, grad, exp_avg, exp_avg_sq, state, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                          grad_scale=1.0, clip_norm=None, clip_value=None, ema=None, ema_decay=0.0):
        """Guarded fused Adam on flat device vectors (in place) + refresh of the engine's weights from ``params``: the gradient is
        scaled by grad_scale, clipped by its norm (clip_norm, torch's clip_grad_norm_) or by value (clip_value, clip_grad_value_);
        a non-finite gradient skips the step on the device (nothing is written, the state block counts it); ``ema`` receives
        ema += (1 - ema_decay) * (p_new - ema).  ``state``: optim_state().  No host synchronisation."""
        if not hasattr(self, "n_params"):
            self.param_layout()
        self._optim_vectors(self.n_params, params, grad, exp_avg, exp_avg_sq, ema, state)
        opts = self._optim_opts(lr, betas, eps, weight_decay, grad_scale, clip_norm, clip_value, ema_decay)
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_adam_step_guarded(self._h, _dptr(params), _dptr(grad), _dptr(exp_avg), _dptr(exp_avg_sq), _dptr(ema),
                                                   _dptr(state), ctypes.byref(opts), _stream_ptr()), "pf_adam_step_guarded")

    def debug_optim_step(self, params, grad, exp_avg, exp_avg_sq, state, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                         grad_scale=1.0, clip_norm=None, clip_value=None, ema=None, ema_decay=0.0):
        """The launches of adam_step_guarded on caller vectors of any length >= 1; the engine's weights are not touched."""
        self._optim_vectors(params.numel(), params, grad, exp_avg, exp_avg_sq, ema, state)
        opts = self._optim_opts(lr, betas, eps, weight_decay, grad_scale, clip_norm, clip_value, ema_decay)
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_debug_optim_step(self._h, params.numel(), _dptr(params), _dptr(grad), _dptr(exp_avg), _dptr(exp_avg_sq),
                                                  _dptr(ema), _dptr(state), ctypes.byref(opts), _stream_ptr()), "pf_debug_optim_step")

    def optim_chunk(self):
        """Elements of the gradient that one workgroup of the guarded step reduces (pf_debug_optim_chunk)."""
        return int(self.lib.pf_debug_optim_chunk())

    def set_train_precision(self, precision):
        """'f32' (default; what the reference trains in) or 'bf16' (the labelled bf16 leg: dense Linears of the message chains'
        forward and of the gradient kernels on bf16 matrix instructions, fp32 accumulation, fp32 master weights)."""
        code = {"f32": 0, "fp32": 0, "float32": 0, "bf16": 1, "bfloat16": 1}.get(str(precision).lower())
        if code is None:
            raise ValueError(f"train precision must be 'f32' or 'bf16', got {precision!r}")
        self._ck(self.lib.pf_train_set_precision(self._h, code), "pf_train_set_precision")

    def train_precision(self):
        out = ctypes.c_int32(0)
        self._ck(self.lib.pf_train_get_precision(self._h, ctypes.byref(out)), "pf_train_get_precision")
        return "bf16" if out.value == 1 else "f32"

    def set_train_family(self, family):
        """'tuned' (default: the gradient path specialised to n_hidden_scalars 128 / vector_size 16; other widths are refused) or
        'wide' (the labelled width-generic leg: training forward and gradient kernels at every supported width pair, 128 / 16
        included, fp32 only).  Inference is unaffected."""
        code = {"tuned": 0, "wide": 1}.get(str(family).lower())
        if code is None:
            raise ValueError(f"train family must be 'tuned' or 'wide', got {family!r}")
        self._ck(self.lib.pf_train_set_family(self._h, code), "pf_train_set_family")

    def train_family(self):
        out = ctypes.c_int32(0)
        self._ck(self.lib.pf_train_get_family(self._h, ctypes.byref(out)), "pf_train_get_family")
        return "wide" if out.value == 1 else "tuned"

    def set_train_input_grads(self, on):
        """Input gradients on the tuned training family (pf_train_set_input_grads; off by default): train_backward(...,
        input_grads=...), input_vjp and guided runs then work on a 128 / 16 handle's tuned kernels, fp32 only.  The wide family
        always has them; switched off, the buffers the switch owns are released."""
        self._ck(self.lib.pf_train_set_input_grads(self._h, 1 if on else 0), "pf_train_set_input_grads")

    def train_input_grads(self):
        out = ctypes.c_int32(0)
        self._ck(self.lib.pf_train_get_input_grads(self._h, ctypes.byref(out)), "pf_train_get_input_grads")
        return bool(out.value)

    GUIDE_FAMILIES = ("wide", "tuned")

    def _check_guide_family(self, guide_family):
        """The kernel family of a guided run's steps: 'wide' (default) or 'tuned' (a 128 / 16 handle's tuned training forward and
        input gradients).  Checked here, before any library call."""
        if guide_family not in self.GUIDE_FAMILIES:
            raise ValueError(f"guide_family must be 'wide' or 'tuned', got {guide_family!r}")
        if guide_family == "tuned" and (self.cfg.n_hidden_scalars, self.cfg.vector_size) != (128, 16):
            raise ValueError("guide_family='tuned' needs the tuned kernels' widths (n_hidden_scalars 128 / vector_size 16); this engine has "
                             f"{self.cfg.n_hidden_scalars} / {self.cfg.vector_size}: use guide_family='wide'")
        return guide_family

    def _arm_guide_family(self, guide_family):
        """Select the training family (and, for 'tuned', the input-gradient switch) of a guided run; returns what to hand to
        _restore_guide_family."""
        before = (self.train_family(), self.train_input_grads())
        if before[0] != guide_family:
            self.set_train_family(guide_family)
        if guide_family == "tuned" and not before[1]:
            self.set_train_input_grads(True)
        return before

    def _restore_guide_family(self, before):
        if self.train_input_grads() != before[1]:
            self.set_train_input_grads(before[1])
        if self.train_family() != before[0]:
            self.set_train_family(before[0])

    @contextlib.contextmanager
    def _armed(self, guide_family, seed, field, feat_norm_constant, restore=True, types=None, pairs=None):
        """What the begin of a run consumes, armed in one order for sample and sample_begin: the training family of a guided run
        (guide_family None: an unguided run, nothing is selected; 'tuned' takes its input-gradient switch along), then the seed
        (seed_next), then the pocket field (field_next), then type guidance (types_next), then pair guidance (pairs_next).  On exit, also on error, family and
        switch are what they were; restore=False leaves them selected (sample_begin: the run's steps need them, its caller
        restores)."""
        before = self._arm_guide_family(guide_family) if guide_family is not None else None
        try:
            if seed is not None:
                self.seed_next(seed[0], seed[1], seed[2], feat_norm_constant)
            if field is not None:
                self.field_next(**field)
            if types is not None:
                self.types_next(**types)
            if pairs is not None:
                self.pairs_next(pairs)
            yield
        finally:
            if restore and before is not None:
                self._restore_guide_family(before)

    def mask_columns(self):
        """columns of a dropout-mask row: n_hidden_scalars + vector_size on the wide training leg, 144 on the tuned one"""
        return self.cfg.n_hidden_scalars + self.cfg.vector_size if self.train_family() == "wide" else 144

    def set_dropout_masks(self, masks):
        """tests: [n_convs, 2, N, S + V] multipliers used instead of the built-in generator (None restores it); S + V = 144 on
        the tuned training leg, n_hidden_scalars + vector_size on the wide one."""
        if masks is not None:
            want = (self.cfg.n_convs, 2, self.Np + self.Nf, self.mask_columns())
            if tuple(masks.shape) != want:
                raise ValueError(f"dropout masks must have shape {want} on the {self.train_family()} training leg, got {tuple(masks.shape)}")
        self._mask_keepalive = None if masks is None else _f32(masks, self.device)
        self._ck(self.lib.pf_debug_set_dropout_masks(self._h, _dptr(self._mask_keepalive)), "pf_debug_set_dropout_masks")

    def dropout_mask(self, layer, which, dropout, seed):
        """[N, S + V] multipliers of conv layer ``layer`` (which: 0 message, 1 residual dropout); rows are global node
        ids (protein atoms first), columns the S scalar features then the V vector channels (128 + 16 on the tuned leg)."""
        out = torch.empty(self.Np + self.Nf, self.mask_columns(), device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_debug_dropout_mask(self._h, layer, which, float(dropout), int(seed) & 0xFFFFFFFF,
                                                    _dptr(out), _stream_ptr()), "pf_debug_dropout_mask")
        return out

    # -- sampling ------------------------------------------------------------------------------
    @staticmethod
    def _struct_array(struct, tabs: Dict[str, torch.Tensor], order):
        """ctypes array of ``struct``, one entry per element of ``order`` (at least one): entry i takes every field from
        tabs[field][order[i]]; an element None leaves its entry zero."""
        order = list(order)
        arr = (struct * max(len(order), 1))()
        for i, s in enumerate(order):
            if s is not None:
                arr[i] = struct(*(float(tabs[f][s]) for f, _ in struct._fields_))
        return arr

    @staticmethod
    def coef_array(coef: Dict[str, torch.Tensor], order):
        """coef: per-s tensors (host logic of the diffusion wrapper); order: iterable of s."""
        return PfEngine._struct_array(L.PfStepCoef, coef, order)

    @staticmethod
    def pin_coef_array(pin_coef: Dict[str, torch.Tensor], order):
        """pin_coef: per-s tensors (schedule.pin_coefficients); order: iterable of s (the same as coef_array's)."""
        return PfEngine._struct_array(L.PfPinCoef, pin_coef, order)

    @staticmethod
    def renoise_coef_array(renoise_coef: Dict[str, torch.Tensor], n=None):
        """renoise_coef: per-pair tensors (schedule.renoise_coefficients); entry i of the array is pair i."""
        return PfEngine._struct_array(L.PfRenoiseCoef, renoise_coef, range(len(renoise_coef["alpha_t_given_s"]) if n is None else n))

    @staticmethod
    def guide_coef_array(guide_coef: Dict[str, torch.Tensor], order):
        """guide_coef: per-s tensors (schedule.guide_coefficients); order: iterable of s (the same as coef_array's)."""
        return PfEngine._struct_array(L.PfGuideCoef, guide_coef, order)

    @staticmethod
    def ms_coef_array(ms_coef: Dict[str, torch.Tensor], order=None):
        """ms_coef: per-step tensors (schedule.multistep_coefficients); entry i of the array is step order[i] (default: every
        step, in order)."""
        return PfEngine._struct_array(L.PfMsCoef, ms_coef, range(len(ms_coef["t"])) if order is None else order)

    @staticmethod
    def plan_arrays(plan, coef, pin_coef, renoise_coef):
        """The four host arrays of pf_sample_pinned_resampled for ``plan`` (schedule.resample_plan): (coef_arr, pin_coef_arr,
        op_arr, renoise_arr), each with one entry per op.  coef / pin_coef: per-s tensors (coef_array / pin_coef_array);
        renoise_coef: schedule.renoise_coefficients of the plan's renoise ops in plan order.  The entries an op's kind does
        not read are zero."""
        for i, op in enumerate(plan):
            if op[0] not in ("denoise", "renoise"):
                raise ValueError(f"op {i} of the plan is {op!r}: expected ('denoise', s) or ('renoise', b, a)")
        steps = [op[1] if op[0] == "denoise" else None for op in plan]
        pairs = iter(range(len(plan)))
        jumps = [next(pairs) if op[0] == "renoise" else None for op in plan]
        op_arr = (ctypes.c_int32 * max(len(plan), 1))(*[int(j is not None) for j in jumps])
        return (PfEngine._struct_array(L.PfStepCoef, coef, steps), PfEngine._struct_array(L.PfPinCoef, pin_coef, steps), op_arr,
                PfEngine._struct_array(L.PfRenoiseCoef, renoise_coef, jumps))

    def _restraint_arrays(self, restraints, tag, tag_first, noun):
        """The one parser of restraint lists: one list (or None) per graph of (tag, center, point, radius, weight) -- center a local center
        index or None / -1 / '*' for every center of the graph, point three coordinates in the caller's frame.  ``tag`` reads the first entry as
        an integer, ``tag_first``: its column stands before the centers', ``noun``: a row in the ValueErrors.  Returns the six host arrays (numpy)."""
        import numpy as np
        if len(restraints) != self.B:
            raise ValueError(f"{noun}s must have one entry per graph ({self.B}), got {len(restraints)}")
        ptr, tags, center, pt, rad, wt = [0], [], [], [], [], []
        for rs in restraints:
            for k, c, p, r, w in (rs or []):
                tags.append(tag(k))
                center.append(-1 if c is None or c == "*" else int(c))
                pt.append([float(v) for v in p])
                if len(pt[-1]) != 3:
                    raise ValueError(f"a {noun}'s point has three coordinates")
                rad.append(float(r)); wt.append(float(w))
            ptr.append(len(tags))
        cols = (tags, center) if tag_first else (center, tags)
        return (np.asarray(ptr, dtype=np.int32), *(np.asarray(c, dtype=np.int32) for c in cols),
                np.ascontiguousarray(np.asarray(pt, dtype=np.float32).reshape(-1, 3)), np.asarray(rad, dtype=np.float32),
                np.asarray(wt, dtype=np.float32))

    def _restraints(self, restraints):
        """restraints: one list (or None) per graph of (kind, center, point, radius, weight) -- kind 'attract' / 'repel' (or 0 / 1).
        Returns the host arrays of pf_sample_begin_guided: ptr, kind, center, point, radius, weight."""
        names = {"attract": 0, "repel": 1, 0: 0, 1: 1}
        def kind(k):
            if isinstance(k, str) and k not in names:
                raise ValueError(f"a restraint's kind is 'attract' or 'repel', got {k!r}")
            return names[k] if k in names else int(k)
        return self._restraint_arrays(restraints, kind, True, "restraint")

    def _free_pins(self):
        """the pin arrays of a run that pins nothing (a guided run is a pinned run whose flags may all be zero)"""
        return (torch.zeros(self.Nf, dtype=torch.int32), torch.zeros(self.Nf, 3), torch.zeros(self.Nf, self.pharm_nf))

    def _pins(self, pins):
        """(flags [Nf] 0..3, positions [Nf,3] in the caller's frame, feature rows [Nf,pharm_nf]) as device tensors."""
        flags, px, ph = pins
        flags = flags.detach().to(self.device, torch.int32).contiguous()
        px, ph = _f32(px, self.device), _f32(ph, self.device)
        if flags.shape != (self.Nf,) or px.shape != (self.Nf, 3) or ph.shape != (self.Nf, self.pharm_nf):
            raise ValueError(f"pins must be (flags [{self.Nf}], positions [{self.Nf}, 3], feature rows [{self.Nf}, {self.pharm_nf}])")
        return flags, px, ph

    def _run_inputs(self, pins, restraints):
        """What a run's kind adds to its begin call, as ctypes arguments: the three device pin arrays (a pinned run; a guided run
        too, all flags zero when it has no pins) and the six host restraint arrays (a guided run).  Returns (pin arguments,
        restraint arguments, the tensors and arrays they point into); a tuple is empty where the kind has none."""
        if pins is None and restraints is None:
            return (), (), ()
        fl = self._pins(pins if pins is not None else self._free_pins())
        rs = self._restraints(restraints) if restraints is not None else ()
        return tuple(_dptr(t) for t in fl), tuple(a.ctypes.data for a in rs), fl + rs

    @staticmethod
    def seed_coef_struct(seed_coef):
        """A PfSeedCoef from schedule.seed_coefficients' dict, an (alpha_a, sigma_a) pair or a PfSeedCoef."""
        if isinstance(seed_coef, L.PfSeedCoef):
            return seed_coef
        if isinstance(seed_coef, dict):
            seed_coef = (seed_coef["alpha_a"], seed_coef["sigma_a"])
        a, sg = seed_coef
        return L.PfSeedCoef(float(a), float(sg))

    def seed_next(self, seed_x, seed_h, seed_coef, feat_norm_constant=1.0):
        """Arms the next begin on this engine -- sample_begin or sample, of any run kind -- with a seed (pf_sample_seed_next): the
        run starts from seed_x [Nf, 3] (caller's frame) / seed_h [Nf, pharm_nf] (raw rows, divided by feat_norm_constant) noised
        to the level of seed_coef (schedule.seed_coefficients) and makes only that level's steps.  That begin consumes the seed,
        accepted or not; a set_batch in between discards it."""
        sx, sh = _f32(seed_x, self.device), _f32(seed_h, self.device)
        if sx.shape != (self.Nf, 3) or sh.shape != (self.Nf, self.pharm_nf):
            raise ValueError(f"a seed is (positions [{self.Nf}, 3], feature rows [{self.Nf}, {self.pharm_nf}])")
        coef = self.seed_coef_struct(seed_coef)
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_sample_seed_next(self._h, ctypes.byref(coef), _dptr(sx), _dptr(sh), float(feat_norm_constant),
                                                  _stream_ptr()), "pf_sample_seed_next")

    def field_next(self, atom_r=None, w_clash=0.0, ph=None, match=None, dist=None, w_comp=0.0, kappa=4.0, type_sharpness=0.0):
        """Arms the next guided begin on this engine -- sample_begin(restraints=...) or sample(restraints=...) -- with a pocket
        field (pf_guide_field_next; the energies: include/pfdyn.h).  atom_r [Np] (or a float for every atom; None: no clash term)
        with w_clash; ph = (ph_ptr [B + 1], ph_x [n, 3] in the caller's frame, ph_type [n]) (None: no complementarity term) with
        match [pharm_nf, pharm_nf] (0 / 1), dist [pharm_nf], w_comp, kappa and type_sharpness.  Host arrays (tensors, numpy or
        lists); the library validates the values (PfError, PF_ERR_ARG) and copies them before this returns.  The begin of any
        other run kind while a field is armed is a PfError (PF_ERR_STATE) and drops it; set_batch drops it silently."""
        import numpy as np
        host = lambda v, d, shape: np.ascontiguousarray(np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=d).reshape(shape))
        keep, none = [], ctypes.c_void_p(None)
        def arg(v, d, shape):
            if v is None:
                return none
            keep.append(host(v, d, shape))
            return keep[-1].ctypes.data
        if atom_r is not None and not torch.is_tensor(atom_r) and np.ndim(atom_r) == 0:
            atom_r = np.full(self.Np, float(atom_r), dtype=np.float32)
        if atom_r is not None:
            atom_r = host(atom_r, np.float32, -1)
            if atom_r.shape[0] != self.Np:
                raise ValueError(f"atom_r has one radius per atom ({self.Np})")
        ptr = xs = ty = None
        if ph is not None:
            ptr, xs, ty = ph
            ptr = host(ptr, np.int32, -1)
            if ptr.shape != (self.B + 1,):
                raise ValueError(f"ph_ptr has B + 1 = {self.B + 1} entries")
            n = max(int(ptr[-1]), 0)
            xs, ty = host(xs, np.float32, (-1, 3)), host(ty, np.int32, -1)
            if xs.shape[0] < n or ty.shape[0] < n:
                raise ValueError(f"ph_ptr names {n} receptor features; ph_x / ph_type hold {xs.shape[0]} / {ty.shape[0]}")
            if match is None or dist is None:
                raise ValueError("receptor features need the match table and the distances")
        nf = self.pharm_nf
        args = (arg(atom_r, np.float32, -1), float(w_clash), arg(ptr, np.int32, -1), arg(xs, np.float32, (-1, 3)), arg(ty, np.int32, -1),
                arg(match, np.int32, (nf, nf)), arg(dist, np.float32, (nf,)), float(w_comp), float(kappa), float(type_sharpness))
        self._ck(self.lib.pf_guide_field_next(self._h, *args), "pf_guide_field_next")

    def last_field_energies(self):
        """[B, 3] of the last guided step with a pocket field: the restraints', the clash and the complementarity energy per
        graph (pf_debug_last_field); their sum in that order is last_guidance()'s E."""
        e3 = torch.empty(self.B, 3, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_debug_last_field(self._h, _dptr(e3), _stream_ptr()), "pf_debug_last_field")
        return e3

    def types_next(self, restraints=None, scale=1.0, clip=0.0, sharpness=0.0, complementarity=False, unmatched=0.0):
        """Arms the next guided begin on this engine with type guidance (pf_guide_types_next; the semantics: include/pfdyn.h):
        the run's feature rows are steered too.  restraints: None, or one list (or None) per graph of (type index, center, point,
        radius, weight) -- center a local center index or None / -1 / '*' for every center of the graph, point three coordinates
        in the caller's frame, radius 0: no spatial condition.  scale / clip: the feature shift's scale and the Euclidean norm a
        row's shift is clipped to (0: no clip); sharpness: that of the soft type assignment (it must equal an armed pocket
        field's); complementarity: the pocket field's complementarity energy also steers the types, a type without a partner in
        the pocket costing ``unmatched``^2.  The library validates the values (PfError, PF_ERR_ARG) and copies them before this
        returns.  The begin of any other run kind while it is armed is a PfError (PF_ERR_STATE) and drops it; set_batch drops it
        silently."""
        keep = self._restraint_arrays(restraints, int, False, "type restraint") if restraints is not None else ()
        args = tuple(a.ctypes.data for a in keep) or (ctypes.c_void_p(None),) * 6
        self._ck(self.lib.pf_guide_types_next(self._h, *args, float(scale), float(clip), float(sharpness), int(bool(complementarity)),
                                              float(unmatched)), "pf_guide_types_next")

    def last_type_guidance(self):
        """(g0_h, grad_h, shift_h [Nf, pharm_nf], E_type [B]) of the last guided step with type guidance
        (pf_debug_last_type_guidance); a type-pinned center's rows are what it ignored."""
        g0, gr, sh = (torch.empty(self.Nf, self.pharm_nf, device=self.device) for _ in range(3))
        en = torch.empty(self.B, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_debug_last_type_guidance(self._h, _dptr(g0), _dptr(gr), _dptr(sh), _dptr(en), _stream_ptr()),
                     "pf_debug_last_type_guidance")
        return g0, gr, sh, en

    def pairs_next(self, restraints=None):
        """Arms the next guided begin on this engine with pair restraints (pf_guide_pairs_next; the semantics: include/pfdyn.h):
        distance restraints between two centers of one graph.  restraints: None, or one list (or None) per graph of
        (i, j, lo, hi, weight) -- i, j local center indices, or None / '*' / a negative index for every center; the energy is
        weight * (max(0, lo - rho)^2 + max(0, rho - hi)^2) on the distance rho of every covered pair, hi = inf: no upper bound.
        The library validates the values (PfError, PF_ERR_ARG) and copies them before this returns.  None, or no restraint in any
        graph, is accepted and inert.  The begin of any other run kind while it is armed is a PfError (PF_ERR_STATE) and drops it;
        set_batch drops it silently."""
        import numpy as np
        if restraints is None:
            args = (ctypes.c_void_p(None),) * 6
            keep = ()
        else:
            if len(restraints) != self.B:
                raise ValueError(f"pair restraints must have one entry per graph ({self.B}), got {len(restraints)}")
            index = lambda c: -1 if c is None or c == "*" or int(c) < 0 else int(c)
            ptr, ci, cj, lo, hi, wt = [0], [], [], [], [], []
            for rs in restraints:
                for row in (rs or []):
                    if len(row) != 5:
                        raise ValueError(f"a pair restraint is (i, j, lo, hi, weight), got {row!r}")
                    i, j, a, b, w = row
                    ci.append(index(i)); cj.append(index(j)); lo.append(float(a)); hi.append(float(b)); wt.append(float(w))
                ptr.append(len(ci))
            keep = (np.asarray(ptr, dtype=np.int32), np.asarray(ci, dtype=np.int32), np.asarray(cj, dtype=np.int32),
                    np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32), np.asarray(wt, dtype=np.float32))
            args = tuple(a.ctypes.data for a in keep)
        self._ck(self.lib.pf_guide_pairs_next(self._h, *args), "pf_guide_pairs_next")     # (keep: the arrays live until here)

    def last_pair_guidance(self):
        """(g_pair [Nf, 3], E_pair [B]) of the last guided step with pair restraints (pf_debug_last_pairs): the pair energies'
        gradient w.r.t. the centers' points (a position-pinned center's row is zero) and their sum per graph."""
        gp = torch.empty(self.Nf, 3, device=self.device)
        en = torch.empty(self.B, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_debug_last_pairs(self._h, _dptr(gp), _dptr(en), _stream_ptr()), "pf_debug_last_pairs")
        return gp, en

    def sample_begin(self, noise0, init_pharm_com=None, pins=None, feat_norm_constant=1.0, restraints=None, guide_scale=1.0,
                     guide_clip=0.0, seed=None, guide_family=None, field=None, types=None, pairs=None):
        """seed = (seed_x, seed_h, seed_coef): seed_next with this call's feat_norm_constant, in front of the begin.
        pins = (flags, positions, feature rows): a pinned run (pf_sample_begin_pinned) -- its steps are
        denoise_step(..., pin_coef=...); feat_norm_constant is what the given feature rows are divided by.
        restraints (one list or None per graph, see _restraints): a guided run (pf_sample_begin_guided) -- its steps are
        guided_step; the caller has selected the wide training family (set_train_family('wide')); pins are optional.
        guide_family 'wide' / 'tuned' (guided runs only; None: the caller has selected the family): selects that training family --
        for 'tuned', a 128 / 16 handle, also the input-gradient switch -- and leaves it selected: the run's steps need it, and the
        caller restores what it had once the run has ended.
        field (a dict of field_next's arguments): a guided run with a pocket field, also without restraints.
        types (a dict of types_next's arguments): a guided run with type guidance, also without restraints.
        pairs (pairs_next's argument): a guided run with pair restraints, also without restraints."""
        if (field is not None or types is not None or pairs is not None) and restraints is None:
            restraints = [None] * self.B
        if guide_family is not None:
            self._check_guide_family(guide_family)
            if restraints is None:
                raise ValueError("guide_family applies to guided runs (restraints=...)")
        nz = _f32(noise0, self.device)
        com = _f32(init_pharm_com, self.device) if init_pharm_com is not None else None
        self._keep = [nz, com]
        pin, restr, _alive = self._run_inputs(pins, restraints)
        with self._armed(guide_family, seed, field, feat_norm_constant, restore=False, types=types, pairs=pairs), torch.cuda.device(self.device):
            if restraints is not None:
                self._ck(self.lib.pf_sample_begin_guided(self._h, _dptr(com), _dptr(nz), *pin, float(feat_norm_constant), *restr,
                                                         float(guide_scale), float(guide_clip), _stream_ptr()), "pf_sample_begin_guided")
            elif pins is not None:
                self._ck(self.lib.pf_sample_begin_pinned(self._h, _dptr(com), _dptr(nz), *pin, float(feat_norm_constant), _stream_ptr()),
                         "pf_sample_begin_pinned")
            else:
                self._ck(self.lib.pf_sample_begin(self._h, _dptr(com), _dptr(nz), _stream_ptr()), "pf_sample_begin")

    def prepare_timesteps(self, coef_arr, n=None):
        """Optional before a loop of denoise_step calls: the timesteps the loop will visit (pf_prepare_timesteps)."""
        n = len(coef_arr) if n is None else n
        tv = (ctypes.c_float * max(n, 1))(*[coef_arr[i].t for i in range(n)])
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_prepare_timesteps(self._h, tv, n, _stream_ptr()), "pf_prepare_timesteps")

    def denoise_step(self, coef_struct, noise, ep_coord=False, ep_feat=False, pin_coef=None):
        """pin_coef (a PfPinCoef, the entry of pin_coef_array for this step): a step of a pinned run."""
        nz = _f32(noise, self.device)
        with torch.cuda.device(self.device):
            if pin_coef is not None:
                self._ck(self.lib.pf_denoise_step_pinned(self._h, ctypes.byref(coef_struct), ctypes.byref(pin_coef), _dptr(nz),
                                                         int(ep_coord), int(ep_feat), _stream_ptr()), "pf_denoise_step_pinned")
                return
            self._ck(self.lib.pf_denoise_step(self._h, ctypes.byref(coef_struct), _dptr(nz), int(ep_coord), int(ep_feat),
                                              _stream_ptr()), "pf_denoise_step")

    def ms_step(self, ms_coef_struct):
        """One multistep step inside a plain run (pf_denoise_step_ms): ms_coef_struct is this step's entry of ms_coef_array.  No
        noise is read.  A non-zero c1 needs a multistep step right in front of it (PfError, PF_ERR_STATE; the run goes on)."""
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_denoise_step_ms(self._h, ctypes.byref(ms_coef_struct), _stream_ptr()), "pf_denoise_step_ms")

    def guided_step(self, coef_struct, pin_coef, guide_coef, noise, ep_coord=False, ep_feat=False):
        """One step of a guided run (pf_denoise_step_guided): coef_struct / pin_coef / guide_coef are this step's entries of
        coef_array / pin_coef_array / guide_coef_array."""
        nz = _f32(noise, self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_denoise_step_guided(self._h, ctypes.byref(coef_struct), ctypes.byref(pin_coef), ctypes.byref(guide_coef),
                                                     _dptr(nz), int(ep_coord), int(ep_feat), _stream_ptr()), "pf_denoise_step_guided")

    def last_guidance(self):
        """(g0 [Nf, 3], grad [Nf, 3], shift [Nf, 3], E [B]) of the last guided step (pf_debug_last_guidance)."""
        g0, gr, sh = (torch.empty(self.Nf, 3, device=self.device) for _ in range(3))
        en = torch.empty(self.B, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_debug_last_guidance(self._h, _dptr(g0), _dptr(gr), _dptr(sh), _dptr(en), _stream_ptr()),
                     "pf_debug_last_guidance")
        return g0, gr, sh, en

    def renoise_step(self, coef, noise):
        """One resampling jump of a pinned run (pf_renoise_step): coef is a PfRenoiseCoef (an entry of renoise_coef_array)."""
        nz = _f32(noise, self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_renoise_step(self._h, ctypes.byref(coef), _dptr(nz), _stream_ptr()), "pf_renoise_step")

    def _sample_outputs(self, frames=0, energy_rows=None):
        """(x [Nf, 3], h [Nf, pharm_nf], trajectory x, trajectory h, energies) on the device; the trajectory arrays have ``frames``
        leading rows (0: None), the energies ``energy_rows`` x B (None: None)."""
        x = torch.empty(self.Nf, 3, device=self.device)
        hh = torch.empty(self.Nf, self.pharm_nf, device=self.device)
        tx = torch.empty(frames, self.Nf, 3, device=self.device) if frames else None
        th = torch.empty(frames, self.Nf, self.pharm_nf, device=self.device) if frames else None
        en = None if energy_rows is None else torch.empty(max(energy_rows, 1), self.B, device=self.device)[:energy_rows]
        return x, hh, tx, th, en

    def sample_end(self, feat_norm_constant=1.0):
        """x_0 / h_0 of the run in progress (pf_sample_end); a pinned run returns its given values bit for bit."""
        x, hh = self._sample_outputs()[:2]
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_sample_end(self._h, float(feat_norm_constant), _dptr(x), _dptr(hh), _stream_ptr()),
                     "pf_sample_end")
        return x, hh

    def sample_frame(self, feat_norm_constant=1.0):
        x, hh = self._sample_outputs()[:2]
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_sample_frame(self._h, float(feat_norm_constant), _dptr(x), _dptr(hh), _stream_ptr()),
                     "pf_sample_frame")
        return x, hh

    def sample(self, coef_arr, n_steps, noise, init_pharm_com=None, ep_coord=False, ep_feat=False,
               feat_norm_constant=1.0, trajectory=False, pins=None, pin_coef_arr=None, plan=None, restraints=None,
               guide_coef_arr=None, guide_scale=1.0, guide_clip=0.0, energies=False, seed=None, ms_coef_arr=None,
               guide_family="wide", field=None, types=None, pairs=None):
        """pairs (pairs_next's argument: one list or None per graph of (i, j, lo, hi, weight)): the guided run carries pair
        restraints; restraints are then optional.
        field (a dict of field_next's arguments): the guided run carries a pocket field; restraints are then optional.
        types (a dict of types_next's arguments): the guided run steers the feature rows too; restraints are then optional.
        seed = (seed_x, seed_h, seed_coef): seed_next with this call's feat_norm_constant, in front of the run -- n_steps is
        then the seed's level a, and coef_arr (and the other per-step arrays) hold the entries of s = a-1 .. 0.
        pins = (flags, positions, feature rows) with pin_coef_arr (pin_coef_array, coef_arr's order): pf_sample_pinned.
        plan = (op_arr, renoise_arr) (plan_arrays; n_steps is then the number of ops and coef_arr / pin_coef_arr have one entry
        per op): pf_sample_pinned_resampled.
        restraints (one list or None per graph, see _restraints) with pin_coef_arr and guide_coef_arr (guide_coef_array): a guided
        run, pf_sample_guided -- pins are optional, a plan is refused.  The run is made on the wide training family; the family
        the engine was on is restored afterwards, also on error.  energies: the restraint energies [n_steps, B] come back
        behind the other outputs.  guide_family='tuned' (a 128 / 16 handle, else ValueError before any call) makes the run on
        the tuned training family with its input-gradient switch armed; family and switch are restored afterwards, also on error.
        ms_coef_arr (ms_coef_array): a multistep run, pf_sample_ms -- coef_arr is not read (None), noise needs its first row only
        (the initial draw), and the parameterisation is in the coefficients; seeds compose, pins, plans and restraints are refused."""
        ms, (op_arr, renoise_arr) = ms_coef_arr is not None, plan or (None, None)
        if (field is not None or types is not None or pairs is not None) and restraints is None and not ms:
            restraints = [None] * self.B
        guided = restraints is not None
        if guide_family not in PfEngine.GUIDE_FAMILIES:
            raise ValueError(f"guide_family must be 'wide' or 'tuned', got {guide_family!r}")
        if ms and (pins is not None or plan is not None or guided or field is not None or types is not None or pairs is not None):
            raise ValueError("a multistep run composes with seeds only: no pins, resampling plan, restraints, pocket field, type or pair guidance")
        if plan is not None and pins is None:
            raise ValueError("a plan needs pins: resampling runs inside a pinned run (all flags zero pins nothing)")
        if guided and plan is not None:
            raise ValueError("guidance together with resampling jumps is not supported")
        if guided and (pin_coef_arr is None or guide_coef_arr is None):
            raise ValueError("a guided run needs pin_coef_arr (PfEngine.pin_coef_array) and guide_coef_arr (PfEngine.guide_coef_array)")
        if pins is not None and pin_coef_arr is None:
            raise ValueError("a pinned run needs pin_coef_arr (PfEngine.pin_coef_array)")
        if guided:
            self._check_guide_family(guide_family)
        kind = "multistep" if ms else "guided" if guided else "resampled" if plan is not None else "pinned" if pins is not None else "plain"
        per_op = {"multistep": dict(ms_coef_arr=ms_coef_arr),
                  "guided": dict(coef_arr=coef_arr, pin_coef_arr=pin_coef_arr, guide_coef_arr=guide_coef_arr),
                  "resampled": dict(coef_arr=coef_arr, pin_coef_arr=pin_coef_arr, op_arr=op_arr, renoise_arr=renoise_arr)}.get(kind, {})
        short = [k for k, a in per_op.items() if len(a) < n_steps]
        if short:
            raise ValueError(f"a {kind} run of {n_steps} ops needs {n_steps} entries in each of its per-op arrays; too short: {', '.join(short)}")
        nz = _f32(noise, self.device)
        if ms and nz.dim() == 2:
            nz = nz[None]
        assert nz.shape[0] >= (1 if ms else n_steps + 1) and nz.shape[1] == self.Nf and nz.shape[2] == 3 + self.pharm_nf
        com = _f32(init_pharm_com, self.device) if init_pharm_com is not None else None
        pin, restr, _alive = self._run_inputs(pins, restraints)
        x0, h0, tx, th, en = self._sample_outputs(n_steps + 1 if trajectory else 0, n_steps if guided and energies else None)
        state, eps = (_dptr(nz), _dptr(com)) + pin, (int(ep_coord), int(ep_feat), float(feat_norm_constant))
        outs = (_dptr(x0), _dptr(h0), _dptr(tx), _dptr(th))
        name, args = {
            "plain": ("pf_sample", (coef_arr,) + state + eps + outs),
            "pinned": ("pf_sample_pinned", (coef_arr, pin_coef_arr) + state + eps + outs),
            "resampled": ("pf_sample_pinned_resampled", (op_arr, coef_arr, pin_coef_arr, renoise_arr) + state + eps + outs),
            "guided": ("pf_sample_guided", (coef_arr, pin_coef_arr, guide_coef_arr) + state + eps + restr
                       + (float(guide_scale), float(guide_clip)) + outs + (_dptr(en) if n_steps else None,)),
            "multistep": ("pf_sample_ms", (ms_coef_arr,) + state + eps[2:] + outs)}[kind]
        with self._armed(guide_family if guided else None, seed, field, feat_norm_constant, types=types, pairs=pairs), torch.cuda.device(self.device):
            self._ck(getattr(self.lib, name)(self._h, n_steps, *args, _stream_ptr()), name)
        out = (x0, h0, tx, th) if trajectory else (x0, h0)
        return out + (en,) if guided and energies else out

    def sample_status(self):
        """Validity of the sampling runs that ended on this handle since the last call (pf_sample_status): raises PfError when a
        hand-over inside a merged launch timed out.  Call once the results have been waited for (stream / event synchronisation)
        and before using them; touches no device."""
        n = ctypes.c_int32()
        self._ck(self.lib.pf_sample_status(self._h, ctypes.byref(n)), "pf_sample_status")

    # -- scoring ------------------------------------------------------------------------------
    def score(self, x0, h0, levels, noise, w_pos, w_feat, alpha_tab, sigma_tab, n_timesteps, feat_norm=1.0, remove_com=True,
              ep_coord=False, ep_feat=False, terms=True):
        """pf_score on the bound batch: the candidates are its centers -- x0 [Nf, 3] in the frame of the bound pockets, h0
        [Nf, pharm_nf] raw type one-hots.  levels: L integers in 0..n_timesteps; noise [L, Nf, 3 + pharm_nf] (x columns first), one
        row per level; w_pos / w_feat: L weights each (schedule.score_weights); alpha_tab / sigma_tab: [n_timesteps + 1].
        Returns (score [B, 2] = sum over levels of w_pos * pos and w_feat * feat, terms [L, B, 4] = pos, feat, err, hits per level
        and graph, or None), device tensors; nothing is divided by the number of centers.  Refused (PfError) while a sampling run
        holds the engine: bind the batch again first."""
        x, hh = _f32(x0, self.device), _f32(h0, self.device)
        lv = [int(t) for t in levels]
        L_ = len(lv)
        if len(w_pos) != L_ or len(w_feat) != L_:
            raise ValueError(f"score: {L_} levels need {L_} weights of each kind, got {len(w_pos)} and {len(w_feat)}")
        nz = _f32(noise, self.device)
        if x.shape != (self.Nf, 3) or hh.shape != (self.Nf, self.pharm_nf) or nz.shape != (L_, self.Nf, 3 + self.pharm_nf):
            raise ValueError(f"score: x0 [{self.Nf}, 3], h0 [{self.Nf}, {self.pharm_nf}] and noise [{L_}, {self.Nf}, {3 + self.pharm_nf}] "
                             f"expected, got {tuple(x.shape)}, {tuple(hh.shape)}, {tuple(nz.shape)}")
        al, sg = _f32(alpha_tab, self.device), _f32(sigma_tab, self.device)
        if al.numel() != n_timesteps + 1 or sg.numel() != n_timesteps + 1:
            raise ValueError(f"score: the alpha / sigma tables have n_timesteps + 1 = {n_timesteps + 1} entries")
        arr = (L.PfScoreLevel * max(L_, 1))(*[L.PfScoreLevel(t, float(a), float(b)) for t, a, b in zip(lv, w_pos, w_feat)])
        score = torch.empty(self.B, 2, device=self.device)
        tm = torch.empty(L_, self.B, 4, device=self.device) if terms else None
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_score(self._h, _dptr(x), _dptr(hh), L_, arr, _dptr(nz), _dptr(al), _dptr(sg), int(n_timesteps),
                                       float(feat_norm), int(bool(remove_com)), int(bool(ep_coord)), int(bool(ep_feat)), _dptr(score),
                                       _dptr(tm), _stream_ptr()), "pf_score")
        return score, tm

    # -- introspection -------------------------------------------------------------------------
    def sample_set(self, x, types, set_ptr, center_ptr, sigma=1.0, tolerance=1.5, threshold=0.5, want_similarity=True):
        """Analyses P sample sets in one call (pf_sample_set_analyze; the definitions: include/pfdyn.h, "sample sets"): the typed
        Gaussian-overlap Tanimoto between the samples of each set, per-center support, Taylor-Butina clusters and the consensus of
        each cluster.  x [N, 3] and types [N] (integers in [0, pharm_nf)) are the centers of all samples, sample s owning rows
        [center_ptr[s], center_ptr[s+1]) and set p the samples [set_ptr[p], set_ptr[p+1]) -- both pointer arrays on the host.
        Returns a dict of device tensors: similarity [sum S_p^2] (the sets' row-major matrices one after the other; None with
        want_similarity=False), support [N], label [S], centroid [S], size [S] (cluster c of set p at set_ptr[p] + c, -1 beyond
        n_clusters), n_clusters [P], cons_x [N, 3], cons_cnt [N].  Needs no weights and no bound batch and touches no run."""
        sp, cp = _i32_host(torch.as_tensor(set_ptr)), _i32_host(torch.as_tensor(center_ptr))
        P = int(sp.shape[0]) - 1
        if P < 1 or sp.ndim != 1 or cp.ndim != 1 or cp.shape[0] < 1:
            raise ValueError("sample_set: set_ptr [P + 1] and center_ptr [S + 1] with at least one set")
        S, N = int(cp.shape[0]) - 1, int(cp[-1])
        if int(sp[-1]) != S:
            raise ValueError(f"sample_set: set_ptr ends at {int(sp[-1])}, center_ptr describes {S} samples")
        xd = _f32(torch.as_tensor(x), self.device).reshape(-1, 3)
        td = torch.as_tensor(types).detach().to(device=self.device, dtype=torch.int32).contiguous().reshape(-1)
        if N < 0 or xd.shape[0] != N or td.shape[0] != N:
            raise ValueError(f"sample_set: center_ptr ends at {N}, x has {xd.shape[0]} rows and types {td.shape[0]}")
        n_sim = sum(int(b - a) ** 2 for a, b in zip(sp[:-1], sp[1:]))
        i32 = lambda n: torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        sim = torch.empty(n_sim, device=self.device) if want_similarity and 0 < n_sim <= L.PF_SSET_MAX_SIM else None
        out = {"similarity": sim, "support": i32(N), "label": i32(S), "centroid": i32(S), "size": i32(S), "n_clusters": i32(P),
               "cons_x": torch.empty(max(N, 1), 3, device=self.device), "cons_cnt": i32(N)}
        opts = L.PfSsetOpts(float(sigma), float(tolerance), float(threshold))
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_sample_set_analyze(self._h, P, sp.ctypes.data, cp.ctypes.data, _dptr(xd), _dptr(td), ctypes.byref(opts),
                                                    _dptr(sim), _dptr(out["support"]), _dptr(out["label"]), _dptr(out["centroid"]),
                                                    _dptr(out["size"]), _dptr(out["n_clusters"]), _dptr(out["cons_x"]),
                                                    _dptr(out["cons_cnt"]), _stream_ptr()), "pf_sample_set_analyze")
        for k, n in (("support", N), ("cons_cnt", N), ("label", S), ("centroid", S), ("size", S)):
            out[k] = out[k][:n]
        out["cons_x"] = out["cons_x"][:N]
        return out

    def align(self, qx, qtypes, q_ptr, lx, ltypes, l_ptr, sigma=1.0, tolerance=1.5, refine=4, min_area=1.0, want_transform=True):
        """Superposes L library entries onto Q queries, every pair, in one call (pf_pharm_align; the definition: include/pfdyn.h,
        "pharmacophore alignment").  qx [Nq, 3] and qtypes [Nq] are the centers of all queries, query k owning rows
        [q_ptr[k], q_ptr[k+1]); lx, ltypes and l_ptr describe the entries likewise -- both pointer arrays on the host, the center
        arrays anywhere (tensors already on the engine's device in fp32 / int32 are passed as they are, so a library is uploaded
        once for many calls).  Returns a dict of device tensors: sim [Q, L], n_matched [Q, L] int32, n_seeds [Q, L] int32 and
        transform [Q, L, 12] (R row-major, then s: entry frame -> query frame; None with want_transform=False).  Needs no weights
        and no bound batch and touches no run."""
        qp, lp = _i32_host(torch.as_tensor(q_ptr)), _i32_host(torch.as_tensor(l_ptr))
        if qp.ndim != 1 or lp.ndim != 1 or qp.shape[0] < 2 or lp.shape[0] < 2:
            raise ValueError("align: q_ptr [Q + 1] and l_ptr [L + 1] with at least one query and one entry")
        Q, Lc = int(qp.shape[0]) - 1, int(lp.shape[0]) - 1
        dev = lambda x, t: (_f32(torch.as_tensor(x), self.device).reshape(-1, 3),
                            torch.as_tensor(t).detach().to(device=self.device, dtype=torch.int32).contiguous().reshape(-1))
        (xq, tq), (xl, tl) = dev(qx, qtypes), dev(lx, ltypes)
        for what, ptr, x, t in (("q", qp, xq, tq), ("l", lp, xl, tl)):
            if int(ptr[-1]) < 0 or x.shape[0] != int(ptr[-1]) or t.shape[0] != int(ptr[-1]):
                raise ValueError(f"align: {what}_ptr ends at {int(ptr[-1])}, the positions have {x.shape[0]} rows and the types {t.shape[0]}")
        n = Q * Lc if Q * Lc <= L.PF_ALIGN_MAX_PAIRS else 1          # (above the cap the library rejects the call: nothing is written)
        out = {"sim": torch.empty(n, device=self.device), "n_matched": torch.empty(n, dtype=torch.int32, device=self.device),
               "n_seeds": torch.empty(n, dtype=torch.int32, device=self.device),
               "transform": torch.empty(n, 12, device=self.device) if want_transform else None}
        opts = L.PfAlignOpts(float(sigma), float(tolerance), int(refine), float(min_area))
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_pharm_align(self._h, Q, qp.ctypes.data, Lc, lp.ctypes.data, _dptr(xq), _dptr(tq), _dptr(xl), _dptr(tl),
                                             ctypes.byref(opts), _dptr(out["sim"]), _dptr(out["n_matched"]), _dptr(out["n_seeds"]),
                                             _dptr(out["transform"]), _stream_ptr()), "pf_pharm_align")
        for k in ("sim", "n_matched", "n_seeds"):
            out[k] = out[k].reshape(Q, Lc)
        if want_transform:
            out["transform"] = out["transform"].reshape(Q, Lc, 12)
        return out

    def get_edges(self, etype: int):
        with torch.cuda.device(self.device):
            n = self._ck(self.lib.pf_debug_get_edges(self._h, etype, None, None, 0, _stream_ptr()), "pf_debug_get_edges")
            src = torch.zeros(max(n, 1), dtype=torch.int32)
            dst = torch.zeros(max(n, 1), dtype=torch.int32)
            self._ck(self.lib.pf_debug_get_edges(self._h, etype, src.data_ptr(), dst.data_ptr(), n, _stream_ptr()),
                     "pf_debug_get_edges")
        return src[:n].long(), dst[:n].long()

    def conv_layer(self, layer, prot_x, pharm_x, h_prot, v_prot, h_pharm, v_pharm):
        a = [_f32(t, self.device) for t in (prot_x, pharm_x, h_prot, v_prot, h_pharm, v_pharm)]
        outs = [torch.empty_like(a[2]), torch.empty_like(a[3]), torch.empty_like(a[4]), torch.empty_like(a[5])]
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_debug_conv_layer(self._h, layer, *[_dptr(t) for t in a], *[_dptr(t) for t in outs],
                                                  _stream_ptr()), "pf_debug_conv_layer")
        return outs

    def work(self):
        """(reference-equivalent flops, bytes, [ff, pf, fp, pp] edge counts) of the last dynamics call."""
        w = self.work_detail()
        return w["flops"], w["bytes"], w["edges"]

    def work_detail(self):
        fl, by, ex = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        ne = (ctypes.c_int64 * 4)()
        el = (ctypes.c_int64 * max(int(self.cfg.n_convs), 1))()
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_debug_work(self._h, ctypes.byref(fl), ctypes.byref(by), ne, ctypes.byref(ex), el,
                                            _stream_ptr()), "pf_debug_work")
        return {"flops": fl.value, "bytes": by.value, "edges": list(ne), "executed_flops": ex.value,
                "executed_edges_per_layer": list(el)}

    def counts(self):
        """Row / edge counts of the last dynamics call: dict(ff, pf, fp, pp, pa, active_atoms, centers, atoms)."""
        out = (ctypes.c_int64 * 8)()
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_debug_counts(self._h, out, _stream_ptr()), "pf_debug_counts")
        return dict(zip(("ff", "pf", "fp", "pp", "pa", "active_atoms", "centers", "atoms"), list(out)))

    def kernel_family(self, layer: int = 0) -> int:
        """Rows per wave of the edge-message launch of `layer` in the last dynamics call: 4 / 8 = row-group kernels
        (k_rg_edge), 16 = 16-row items on four waves (k_n16_edge; 17: the fused launch k_n16_fused, which also computes conv layer 0's
        node update of its source rows), 32 = one wave per tile (k_edge_msg), 128 = four waves per tile (k_edge_msg_coop)."""
        r = ctypes.c_int32()
        self._ck(self.lib.pf_debug_kernel_family(self._h, int(layer), ctypes.byref(r)), "pf_debug_kernel_family")
        return int(r.value)

    def last_eps(self):
        """(eps_h, eps_x) of the last denoising step's dynamics call."""
        eh = torch.empty(self.Nf, self.pharm_nf, device=self.device); ex = torch.empty(self.Nf, 3, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_debug_last_eps(self._h, _dptr(eh), _dptr(ex), _stream_ptr()), "pf_debug_last_eps")
        return eh, ex

    def xchg_timeouts(self) -> int:
        """Time-outs of the merged last launch's exchange (k_rg_node_hs_build) since the handle was created; synchronises the device.
        The product-path check is sample_status()."""
        r = ctypes.c_int32()
        self._ck(self.lib.pf_debug_xchg_timeouts(self._h, ctypes.byref(r)), "pf_debug_xchg_timeouts")
        return int(r.value)

    @staticmethod
    def live_memory():
        """(allocations, bytes) this process holds through the library's handles right now, device and pinned memory together
        (pf_debug_live_memory): every engine counts, other processes on the device do not."""
        n, b = ctypes.c_int64(), ctypes.c_int64()
        if L.load().pf_debug_live_memory(ctypes.byref(n), ctypes.byref(b)) < 0:
            raise L.PfError("pf_debug_live_memory failed")
        return int(n.value), int(b.value)

    def xchg_fault(self, drop_word: bool, poll_max: int = 0):
        """Diagnostic (pf_debug_xchg_fault): make the merged launch's producers skip one exchange word / shorten the poll bound."""
        self._ck(self.lib.pf_debug_xchg_fault(self._h, int(bool(drop_word)), int(poll_max)), "pf_debug_xchg_fault")

    def ahead(self):
        """What the last denoising step's merged launch did ahead for the next call (pf_debug_ahead): dict(pa_skipped, pa_ahead,
        center_hoist, centers)."""
        out = (ctypes.c_int64 * 4)()
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_debug_ahead(self._h, out, _stream_ptr()), "pf_debug_ahead")
        return dict(zip(("pa_skipped", "pa_ahead", "center_hoist", "centers"), list(out)))

    def pa_check_counts(self):
        """The check of the rows computed ahead (pf_debug_pa_check; PFDYN_PA_CHECK=1 when the handle was created), cumulative:
        dict(violations = kept "pa" groups the previous step's speculative items did not compute, checked = kept groups checked,
        exposed = kept groups of a graph behind a changed group count of an earlier graph)."""
        out = (ctypes.c_int64 * 3)()
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_debug_pa_check(self._h, out, _stream_ptr()), "pf_debug_pa_check")
        return dict(zip(("violations", "checked", "exposed"), list(out)))

    def pa_check(self) -> int:
        """Violations counted by the check of the rows computed ahead (see pa_check_counts)."""
        return self.pa_check_counts()["violations"]

    def l0_hoist(self) -> int:
        """Rows per hoisted wave of conv layer 0's pp messages in the last dynamics call (0: static hoist not used)."""
        r = ctypes.c_int32()
        self._ck(self.lib.pf_debug_l0_hoist(self._h, ctypes.byref(r)), "pf_debug_l0_hoist")
        return int(r.value)

    def debug_chain(self, kind: int, layer: int, sub: int, s_in: torch.Tensor, v_in: torch.Tensor):
        """pf_debug_chain: one chain of the row-group kernels on the given rows (kinds and shapes: include/pfdyn.h)."""
        s_in = s_in.to(self.device, torch.float32).contiguous()
        v_in = v_in.to(self.device, torch.float32).contiguous()
        n = s_in.shape[0]
        if kind == 3:
            s_out = torch.empty(n, self.cfg.pharm_nf, device=self.device)
            v_out = torch.empty(n, 3, device=self.device)
        else:
            s_out = torch.empty(n, 128, device=self.device)
            v_out = torch.empty(n, 16, 3, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_debug_chain(self._h, int(kind), int(layer), int(sub), int(n), _dptr(s_in), _dptr(v_in),
                                             _dptr(s_out), _dptr(v_out), _stream_ptr()), "pf_debug_chain")
        return s_out, v_out

    KERNEL_CLASSES = ("encode", "build_edges", "edge_msg", "node_update", "noise_head", "step_update", "edge_msg_coop",
                      "node_update_coop", "edge_msg_last")

    def profile_enable(self, mask: int):
        self._ck(self.lib.pf_profile_enable(self._h, mask), "pf_profile_enable")

    TRAIN_KERNEL_CLASSES = ("bwd_head", "bwd_node", "bwd_edge_level", "bwd_rest")

    def profile_read_train(self):
        """{gradient-kernel class: (total device ms, launches)} since the last read (profile_enable bits 9..12)."""
        ms = (ctypes.c_double * 4)()
        n = (ctypes.c_int64 * 4)()
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_profile_read_train(self._h, ms, n, _stream_ptr()), "pf_profile_read_train")
        return {k: (ms[i], n[i]) for i, k in enumerate(self.TRAIN_KERNEL_CLASSES)}

    def profile_read(self):
        """{kernel class: (total device ms, launches)} since the last enable/read (synchronises)."""
        ms = (ctypes.c_double * 9)()
        n = (ctypes.c_int64 * 9)()
        with torch.cuda.device(self.device):
            self._ck(self.lib.pf_profile_read(self._h, ms, n, _stream_ptr()), "pf_profile_read")
        return {k: (ms[i], n[i]) for i, k in enumerate(self.KERNEL_CLASSES)}
