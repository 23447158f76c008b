"""Host-side mirror of the reference's model classes for the denoising path.

The nn.Module tree below reproduces the reference's *parameter layout* (so ``state_dict()`` /
``load_state_dict()`` / Lightning ``.ckpt`` files use exactly the reference key set, SURVEY.md
section 5) and its *call surface*:

    PharmRecDynamicsGVP.forward(g, timestep, batch_idxs)      pharmacoforge/models/dynamics_gvp.py:131
    PharmacophoreDiff.sample_given_receptor / sample / forward  pharmacoforge/models/pharmacodiff.py:433,516,162

but none of these modules computes anything in PyTorch: every forward -- and, in training, the
backward of the dynamics -- goes through libpfdyn.so (csrc/, C ABI in include/pfdyn.h); PyTorch
supplies the autograd plumbing around it, the elementwise loss and the optimiser.  There is no
eager / CPU fallback -- without the HIP library and a GPU the calls raise.
"""
from __future__ import annotations

import contextlib
import dataclasses
import math
import warnings
from math import ceil
from pathlib import Path
from typing import Dict, List, Optional, Union

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .analysis import PharmacophoreScore, SampleAnalyzer, SampledPharmacophore, pair_restraint_energy
from .analysis import SampleSet, _sset_options, _sset_samples, analyze_sample_set
from .analysis import (ALIGN_MAX_PAIRS, PharmacophoreLibrary, ScreenHit, _align_options, _align_queries, align_pharmacophores)
from ._lib import PF_SSET_MAX_SIM as SSET_MAX_SIM      # floats of all similarity matrices of one pf_sample_set_analyze call
from .engine import PfEngine
from .graph import PocketGraph, as_pocket_graph, batch as batch_graphs, copy_graph, get_batch_idxs, unbatch
from .schedule import score_levels as _score_levels, score_weights as _score_weights
from .schedule import (PredefinedNoiseSchedule, alpha as _alpha, guide_coefficients, pin_coefficients, renoise_coefficients, resample_plan,
                       seed_coefficients, sigma as _sigma, sigma_and_alpha_t_given_s, step_coefficients)
from .schedule import level_plan, multistep_coefficients, strided_coefficients

try:  # subclass LightningModule when Lightning is importable (drop-in for train.py / load_from_checkpoint)
    import pytorch_lightning as pl
    _Base = pl.LightningModule
except Exception:  # Lightning absent (this image): same surface on top of nn.Module
    pl = None
    _Base = nn.Module


# ---------------------------------------------------------------------------------------------
# parameter containers with the reference's names (gvp.py:43-166, 343-437; dynamics_gvp.py:10-129)
# ---------------------------------------------------------------------------------------------
class GVP(nn.Module):
    def __init__(self, dim_vectors_in, dim_vectors_out, dim_feats_in, dim_feats_out, hidden_vectors=None,
                 feats_activation=None, vectors_activation=None, vector_gating=True, xavier_init=False):
        super().__init__()
        if not vector_gating:
            raise NotImplementedError("only vector-gated GVPs are on the hot path (gvp.py:79-80)")
        self.dim_vectors_in, self.dim_feats_in, self.dim_vectors_out = dim_vectors_in, dim_feats_in, dim_vectors_out
        dim_h = max(dim_vectors_in, dim_vectors_out) if hidden_vectors is None else hidden_vectors
        wh_k, wu_k = 1 / math.sqrt(dim_vectors_in), 1 / math.sqrt(dim_h)
        self.Wh = nn.Parameter(torch.zeros(dim_vectors_in, dim_h).uniform_(-wh_k, wh_k))
        self.Wu = nn.Parameter(torch.zeros(dim_h, dim_vectors_out).uniform_(-wu_k, wu_k))
        self.to_feats_out = nn.Sequential(nn.Linear(dim_h + dim_feats_in, dim_feats_out), nn.SiLU())
        self.scalar_to_vector_gates = nn.Linear(dim_feats_out, dim_vectors_out)
        if xavier_init:
            nn.init.xavier_uniform_(self.scalar_to_vector_gates.weight, gain=1)
            nn.init.constant_(self.scalar_to_vector_gates.bias, 0)


class _VDropout(nn.Module):
    def __init__(self, drop_rate):
        super().__init__()
        self.drop_rate = drop_rate
        self.dummy_param = nn.Parameter(torch.empty(0))      # the reference's empty tensor, kept for key parity


class GVPDropout(nn.Module):
    def __init__(self, rate):
        super().__init__()
        self.vector_dropout = _VDropout(rate)
        self.feat_dropout = nn.Dropout(rate)


class GVPLayerNorm(nn.Module):
    def __init__(self, feats_h_size, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.feat_norm = nn.LayerNorm(feats_h_size)


class GVPMultiEdgeConv(nn.Module):
    def __init__(self, etypes, scalar_size=128, vector_size=16, n_message_gvps=1, n_update_gvps=1, rbf_dmax=15,
                 rbf_dim=16, message_norm: Union[float, str, Dict] = 10, dropout=0.0):
        super().__init__()
        self.etypes = etypes
        self.dst_ntypes = sorted(set(e[2] for e in etypes))
        if isinstance(message_norm, str) and message_norm != 'mean':
            raise ValueError(f"message_norm values must be 'mean' or a positive number, got {message_norm}")
        if isinstance(message_norm, (int, float)) and message_norm < 0:
            raise ValueError(f"message_norm values must be 'mean' or a positive number, got {message_norm}")
        self.edge_message_fns = nn.ModuleDict()
        for etype in etypes:
            gvps = []
            for i in range(n_message_gvps):
                vi = vector_size + 1 if i == 0 else vector_size
                si = scalar_size + rbf_dim if i == 0 else scalar_size
                gvps.append(GVP(vi, vector_size, si, scalar_size))
            self.edge_message_fns['_'.join(etype)] = nn.Sequential(*gvps)
        self.node_update_fns = nn.ModuleDict()
        self.update_layer_norms = nn.ModuleDict()
        self.message_layer_norms = nn.ModuleDict()
        for ntype in self.dst_ntypes:
            self.node_update_fns[ntype] = nn.Sequential(*[GVP(vector_size, vector_size, scalar_size, scalar_size)
                                                          for _ in range(n_update_gvps)])
            self.message_layer_norms[ntype] = GVPLayerNorm(scalar_size)
            self.update_layer_norms[ntype] = GVPLayerNorm(scalar_size)
        self.dropout = GVPDropout(dropout)


class NoisePredictionBlock(nn.Module):
    def __init__(self, in_scalar_dim, out_scalar_dim, vector_size, n_gvps=3, intermediate_scalar_dim=64):
        super().__init__()
        gvps = []
        for i in range(n_gvps):
            last = i == n_gvps - 1
            gvps.append(GVP(vector_size, 1 if last else vector_size, in_scalar_dim,
                            intermediate_scalar_dim if last else in_scalar_dim))
        self.gvps = nn.Sequential(*gvps)
        self.to_scalar_output = nn.Linear(intermediate_scalar_dim, out_scalar_dim)


class PharmRecGVP(nn.Module):
    pharmacophore_edges = [('pharm', 'ff', 'pharm'), ('prot', 'pf', 'pharm')]
    protein_edges = [('pharm', 'fp', 'prot'), ('prot', 'pp', 'prot')]
    all_edges = pharmacophore_edges + protein_edges

    def __init__(self, in_scalar_dim, in_vector_dim, out_scalar_dim, n_convs=4, n_message_gvps=3, n_update_gvps=2,
                 message_norm=10, n_noise_gvps=3, dropout=0.0):
        super().__init__()
        self.conv_layers = nn.ModuleList([
            GVPMultiEdgeConv(self.all_edges, in_scalar_dim, in_vector_dim, n_message_gvps, n_update_gvps,
                             message_norm=message_norm, dropout=dropout) for _ in range(n_convs)])
        self.noise_predictor = NoisePredictionBlock(in_scalar_dim, out_scalar_dim, in_vector_dim, n_noise_gvps)


_warned_no_input_grads = False


class _DynamicsFn(torch.autograd.Function):
    """PharmRecDynamicsGVP.forward as one autograd node: forward = pf_train_forward (train-mode dropout inside the
    kernels), backward = pf_train_backward, which returns d(loss)/d(parameter) for every parameter as one flat vector.
    x_t and h_t get their gradient too when they require one and the engine is on the wide training family
    (set_train_family('wide'): pf_train_backward_inputs) or on the tuned one with set_train_input_grads(True); on the tuned
    family without that switch they get None, with one warning per process.  The edge sets are piecewise constant in x_t and carry no gradient, as in the reference; t and the protein
    coordinates get none."""

    @staticmethod
    def forward(ctx, mod, eng, x_t, h_t, t, prot_x, dropout, seed, flat_leaf):
        eps_h, eps_x = eng.train_forward(x_t, h_t, t, prot_x=prot_x, dropout=dropout, seed=seed)
        mod._fwd_token += 1
        ctx.mod, ctx.eng, ctx.token = mod, eng, mod._fwd_token
        ctx.in_like = tuple((a.shape, a.dtype, a.device) if torch.is_tensor(a) else None for a in (x_t, h_t))
        return eps_h, eps_x

    @staticmethod
    def backward(ctx, g_h, g_x):
        global _warned_no_input_grads
        mod, eng = ctx.mod, ctx.eng
        if ctx.token != mod._fwd_token:
            raise RuntimeError("backward of a PharmRecDynamicsGVP call that is not the most recent training forward: "
                               "the engine keeps the activations of one forward at a time")
        g_h = torch.zeros(eng.Nf, eng.pharm_nf, device=eng.device) if g_h is None else g_h.contiguous()
        g_x = torch.zeros(eng.Nf, 3, device=eng.device) if g_x is None else g_x.contiguous()
        # ONE gradient for autograd: the flat vector, for the flat leaf that aliases every parameter (244 separate
        # gradient views and AccumulateGrad nodes cost 1.4 ms of host time per step -- more than the device could hide);
        # the hooks of the leaf re-bind each parameter's .grad to its slice (PharmRecDynamicsGVP._bind_grads)
        want = (ctx.needs_input_grad[2], ctx.needs_input_grad[3])
        if not any(want):
            return (None,) * 8 + (eng.train_backward(g_h, g_x),)
        if eng.train_family() != "wide" and not eng.train_input_grads():
            if not _warned_no_input_grads:
                _warned_no_input_grads = True
                warnings.warn("x_t / h_t require a gradient, but the tuned training family computes parameter gradients only: "
                              "they get none.  set_train_family('wide') selects the family that differentiates the inputs; "
                              "set_train_input_grads(True) makes the tuned family do it.")
            return (None,) * 8 + (eng.train_backward(g_h, g_x),)
        grads = eng.train_backward(g_h, g_x, input_grads=want)
        g_in = [None if g is None else g.to(device=like[2], dtype=like[1]).reshape(like[0])
                for g, like in zip(grads[1:], ctx.in_like)]
        return (None, None, g_in[0], g_in[1], None, None, None, None, grads[0])


class _LossFn(torch.autograd.Function):
    """PharmacophoreDiff.forward's loss (pharmacodiff.py:162-243, either parameterisation of either output) as one autograd node:
    forward = pf_train_loss_forward_ep (COM removal, noising, train-mode dynamics, losses and metrics on the device), backward =
    pf_train_loss_backward_out with the upstream gradient of the output vector.  Output: [pos loss, feat loss, four metrics,
    total loss, total error, weighted total error]."""

    @staticmethod
    def forward(ctx, mod, eng, x0, h0, t_int, eps_x, eps_h, tabs, T, feat_norm, remove_com, weighted, dropout, seed, ep_coord,
                ep_feat, flat_leaf):
        out = eng.train_loss_forward(x0, h0, t_int, eps_x, eps_h, tabs[0], tabs[1], T, feat_norm, remove_com, weighted,
                                     dropout=dropout, seed=seed, ep_coord=ep_coord, ep_feat=ep_feat)
        mod._fwd_token += 1
        ctx.mod, ctx.eng, ctx.token = mod, eng, mod._fwd_token
        ctx.set_materialize_grads(False)
        # second output: the total loss (entry 6) as a 0-dim tensor of its own -- a step that differentiates only the total loss
        # then hands its upstream scalar straight to the C ABI instead of scattering it into a [9] vector first (a zero fill and
        # a copy launch per step)
        return out, out[6]

    @staticmethod
    def backward(ctx, g_out, g_total):
        mod, eng = ctx.mod, ctx.eng
        if ctx.token != mod._fwd_token:
            raise RuntimeError("backward of a loss forward that is not the most recent training forward: the engine keeps "
                               "the activations of one forward at a time")
        if g_out is None and g_total is None:
            return (None,) * 17
        leaf = mod.__dict__.get("_flat_leaf")
        # FlatAdam.zero_grad(lazy=True) left the clear to this backward: the gradient kernels STORE every element, so writing
        # into the bound flat gradient is the clear and the accumulation at once (no fill, no add: two 3 MB launches per step);
        # the parameters' .grad views stay bound, the accumulate hooks are not needed (no gradient is returned for the leaf)
        into = leaf.grad if (mod.__dict__.get("_grad_lazy_zero") and leaf is not None and leaf.grad is not None) else None
        if g_out is None:
            g = eng.train_loss_backward(g_total, g_total, out=into)          # total loss = pos loss + feat loss
        else:
            if g_total is not None:
                g_out = g_out.clone()
                g_out[6] += g_total
            g = eng.train_loss_backward_out(g_out, out=into)
        if into is not None:
            mod.__dict__["_grad_lazy_zero"] = False
            mod._last_flat_grad = into
            return (None,) * 17
        return (None,) * 16 + (g,)


class PharmRecDynamicsGVP(nn.Module):
    """Drop-in for pharmacoforge.models.dynamics_gvp.PharmRecDynamicsGVP (same constructor, same
    state-dict keys, same forward signature); forward runs on the MI355X through libpfdyn."""

    def __init__(self, n_pharm_scalars, n_prot_scalars, vector_size: int = 16, n_convs=4, n_hidden_scalars=128,
                 act_fn=nn.SiLU, message_norm=1, graph_cutoffs: dict = {}, n_message_gvps: int = 3,
                 n_update_gvps: int = 2, n_noise_gvps: int = 3, dropout: float = 0.0, ff_k: int = 0, pf_k: int = 0):
        super().__init__()
        self.graph_cutoffs = graph_cutoffs
        self.n_pharm_scalars, self.n_prot_scalars = n_pharm_scalars, n_prot_scalars
        self.vector_size, self.ff_k, self.pf_k = vector_size, ff_k, pf_k
        self._arch = dict(pharm_nf=n_pharm_scalars, rec_nf=n_prot_scalars, vector_size=vector_size,
                          n_hidden_scalars=n_hidden_scalars, n_convs=n_convs, n_message_gvps=n_message_gvps,
                          n_update_gvps=n_update_gvps, n_noise_gvps=n_noise_gvps, message_norm=message_norm,
                          ff_k=ff_k, pf_k=pf_k, graph_cutoffs=dict(graph_cutoffs))
        self.dropout_rate = dropout
        self.pharm_encoder = nn.Sequential(nn.Linear(n_pharm_scalars + 1, n_hidden_scalars), act_fn(),
                                           nn.LayerNorm(n_hidden_scalars))
        self.prot_encoder = nn.Sequential(nn.Linear(n_prot_scalars + 1, n_hidden_scalars), act_fn(),
                                          nn.LayerNorm(n_hidden_scalars))
        self.noise_predictor = PharmRecGVP(n_hidden_scalars, vector_size, n_pharm_scalars, n_convs, n_message_gvps,
                                           n_update_gvps, message_norm, n_noise_gvps, dropout)
        self._engine: Optional[PfEngine] = None
        self._weights_stamp = None
        self._batch_key = None
        self._bound_static = None                       # strong references to the tensors behind _batch_key
        self._flat: Optional[torch.Tensor] = None       # all parameters as one device vector (engine layout)
        self._flat_views = []                           # [(parameter, offset, numel)] in that layout
        self._fwd_token = 0

    # -- engine plumbing ------------------------------------------------------------------
    def _device(self) -> torch.device:
        return next(self.parameters()).device

    def engine(self) -> PfEngine:
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError("PharmRecDynamicsGVP runs only on an MI355X (move the model to 'cuda'); "
                               "there is no CPU fallback")
        if self._engine is None or self._engine.device != dev:
            self._engine = PfEngine(device=dev, **self._arch)
            self._engine.set_train_precision(getattr(self, "train_precision", "f32"))
            self._engine.set_train_family(getattr(self, "train_family", "tuned"))
            self._engine.set_train_input_grads(getattr(self, "train_input_grads", False))
            self._join_prefetch()
            self.__dict__["_twin"] = None           # (prefetch_graph makes a new one on this device)
            self._weights_stamp = None
            self._batch_key = None
            self._flat = None
        if self._flat is None or not self._views_intact():
            # first use on this device (or the parameters were re-allocated, e.g. by .to()): push the tensors through
            # the C ABI once, then re-home every parameter as a view of one flat device vector in the engine's
            # layout, so that an optimiser step is visible to the engine as a single device-to-device refresh
            self._engine.load_state_dict({k: v for k, v in self.state_dict().items()}, prefix="")
            self._flatten_parameters()
            self._weights_stamp = self._stamp()
        stamp = self._stamp()
        if stamp != self._weights_stamp:       # parameters were updated in place (optimiser step, load_state_dict)
            self._engine.set_flat_params(self._flat)
            self._weights_stamp = stamp
        return self._engine

    def set_train_precision(self, precision: str):
        """'f32' (default: what the reference trains in) or 'bf16' -- the labelled bf16 training leg (dense Linears of the message
        chains' forward and of the gradient kernels on bf16 matrix instructions, fp32 accumulation, fp32 master weights and
        optimiser).  No reference counterpart; inference is unaffected."""
        if str(precision).lower() not in ("f32", "fp32", "float32", "bf16", "bfloat16"):
            raise ValueError(f"train precision must be 'f32' or 'bf16', got {precision!r}")
        self.train_precision = "bf16" if str(precision).lower() in ("bf16", "bfloat16") else "f32"
        if self._engine is not None:
            self._engine.set_train_precision(self.train_precision)
        twin = self.__dict__.get("_twin")
        if twin is not None:
            self._join_prefetch()
            twin.set_train_precision(self.train_precision)

    def set_train_family(self, family: str):
        """'tuned' (default: the gradient kernels specialised to n_hidden_scalars 128 / vector_size 16) or 'wide' -- the labelled
        width-generic training leg (fp32 only), which trains at every supported width pair.  Inference is unaffected."""
        if str(family).lower() not in ("tuned", "wide"):
            raise ValueError(f"train family must be 'tuned' or 'wide', got {family!r}")
        self.train_family = str(family).lower()
        if self._engine is not None:
            self._engine.set_train_family(self.train_family)
        twin = self.__dict__.get("_twin")
        if twin is not None:
            self._join_prefetch()
            twin.set_train_family(self.train_family)

    def set_train_input_grads(self, on: bool):
        """Input gradients on the tuned training family (off by default): with it on, x_t / h_t that require a gradient get one
        from the tuned kernels (fp32 only), as they do on the wide family.  Off, the tuned family gives them None with one
        warning per process."""
        self.train_input_grads = bool(on)
        if self._engine is not None:
            self._engine.set_train_input_grads(self.train_input_grads)
        twin = self.__dict__.get("_twin")
        if twin is not None:
            self._join_prefetch()
            twin.set_train_input_grads(self.train_input_grads)

    def lane_engine(self, lane: int) -> PfEngine:
        """Engine of sampling lane ``lane``: lane 0 is engine(); further lanes are extra handles (own workspace) that carry
        the same weights -- PharmacophoreDiff.sample keeps several batches in flight on as many HIP streams, because most
        launches of a batched step leave part of the chip idle.  Call under the lane's stream."""
        eng0 = self.engine()
        if lane == 0:
            return eng0
        extra = self.__dict__.setdefault("_lane_engines", {})
        ent = extra.get(lane)
        if ent is None or ent[0].device != eng0.device:
            eng = PfEngine(device=eng0.device, **self._arch)
            eng.load_state_dict({k: v for k, v in self.state_dict().items()}, prefix="")
            ent = [eng, None]
            extra[lane] = ent
        if ent[1] != self._weights_stamp:
            ent[0].set_flat_params(self._flat)
            ent[1] = self._weights_stamp
        return ent[0]

    def _stamp(self):
        return tuple(p._version for p, _, _ in self._flat_views)

    def _named_views(self):
        """[(parameter name, parameter)] in the order of _flat_views"""
        name_of = {id(p): k for k, p in self.named_parameters()}
        return [(name_of[id(p)], p) for p, _, _ in self._flat_views]

    def _views_intact(self) -> bool:
        # (an address inside the flat vector's allocation implies its device)
        base = self._flat.data_ptr()
        return all(p.data_ptr() == base + 4 * off for p, off, _ in self._flat_views)

    def _flatten_parameters(self):
        eng = self._engine
        layout = eng.param_layout()
        flat = torch.empty(eng.n_params, device=eng.device)
        named = dict(self.named_parameters())
        views = []
        for name, off, n in layout:
            p = named[name[len("dynamics."):]]
            flat[off:off + n].copy_(p.data.reshape(-1))
            p.data = flat[off:off + n].view(p.shape)
            views.append((p, off, n))
        self._flat, self._flat_views = flat, views
        # the autograd face of the parameters: one leaf over the same storage (not a registered parameter: state_dict and
        # parameters() keep the reference's 244 tensors).  Its incoming-gradient hook notices gradients that were
        # cleared parameter by parameter (optimizer.zero_grad(), module.zero_grad()), its post-accumulate hook points
        # every parameter's .grad at its slice of the accumulated flat gradient.
        leaf = flat.detach().requires_grad_(True)
        leaf.register_hook(self._before_accumulate)
        leaf.register_post_accumulate_grad_hook(self._bind_grads)
        self.__dict__["_flat_leaf"] = leaf
        self._last_flat_grad = None
        # a gradient that reaches a parameter DIRECTLY (a regulariser on p, any loss term outside the fused nodes) accumulates
        # into p.grad -- a view of the flat gradient -- without passing the leaf: a deferred clear (FlatAdam.zero_grad(lazy=True))
        # has to happen in front of that too, whichever of the two arrives first in a backward
        for p, _, _ in views:
            if p.requires_grad and not getattr(p, "_pf_lazy_hook", False):
                p.register_hook(self._param_grad_arrives)
                p._pf_lazy_hook = True

    def _param_grad_arrives(self, grad):
        if self.__dict__.get("_grad_lazy_zero"):
            self.__dict__["_grad_lazy_zero"] = False
            leaf = self.__dict__.get("_flat_leaf")
            if leaf is not None and leaf.grad is not None:
                leaf.grad.zero_()
        return grad

    def _before_accumulate(self, grad):
        leaf = self.__dict__["_flat_leaf"]
        if self.__dict__.get("_grad_lazy_zero"):        # a deferred clear (FlatAdam.zero_grad(lazy=True)) met by a backward that accumulates
            self.__dict__["_grad_lazy_zero"] = False
            if leaf.grad is not None:
                leaf.grad.zero_()
        if leaf.grad is not None:
            p0 = next((p for p, _, _ in self._flat_views if p.requires_grad), None)
            if p0 is None or p0.grad is None or p0.grad.data_ptr() != leaf.grad.data_ptr() + 4 * next(o for q, o, _ in self._flat_views if q is p0):
                leaf.grad = None                # the per-parameter gradients were cleared or replaced: start afresh
        return grad

    def _bind_grads(self, leaf):
        g = leaf.grad
        self._last_flat_grad = g
        p0, o0 = next(((p, o) for p, o, _ in self._flat_views if p.requires_grad), (None, 0))
        if p0 is not None and p0.grad is not None and p0.grad.data_ptr() == g.data_ptr() + 4 * o0:
            return                              # accumulated in place: the views are still the gradient
        for p, off, n in self._flat_views:
            if p.requires_grad:
                p.grad = g[off:off + n].view(p.shape)

    def allreduce_gradients(self, group=None, average: bool = True):
        """Data-parallel training (one process per GPU): sum the gradients of all ranks with ONE all-reduce of the
        flat gradient vector (3.1 MB at dev.yml; RCCL when the tensors are on the GPU), then re-bind every
        parameter's .grad to its slice.  SURVEY.md 8(e)."""
        import torch.distributed as dist

        def reduce_(t):
            if t.is_cuda and dist.get_backend(group) != "nccl":      # gloo dry runs (ranks sharing a card): via the host
                c = t.cpu()
                dist.all_reduce(c, group=group)
                t.copy_(c)
            else:
                dist.all_reduce(t, group=group)
        params = [p for p, _, _ in self._flat_views] or [p for p in self.parameters() if p.numel() > 0]
        flat = getattr(self, "_last_flat_grad", None)
        off0 = self._flat_views[0][1] if self._flat_views else 0
        if flat is not None and params and params[0].grad is not None and params[0].grad.data_ptr() == flat.data_ptr() + 4 * off0:
            reduce_(flat)                        # the parameters' .grad are views of this vector already
            if average:
                flat /= dist.get_world_size(group)
            return flat
        flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in params])
        reduce_(flat)
        if average:
            flat /= dist.get_world_size(group)
        off = 0
        for p in params:
            p.grad = flat[off:off + p.numel()].view(p.shape)
            off += p.numel()
        self._last_flat_grad = flat
        return flat

    def bind_graph(self, g: PocketGraph, prot_x: Optional[torch.Tensor] = None) -> PfEngine:
        """Upload the static part of a batch (pocket atoms, pp edges, graph boundaries) once.

        The upload is skipped only when the very same tensors are bound again: the key holds the storage address and
        version counter of every static tensor plus the ptr arrays' contents, and the module keeps a strong reference
        to those tensors while they are bound -- so neither CPython nor the caching allocator can hand their addresses
        to another batch (a temporary such as ``training_step(g.to(dev))`` is kept alive until the next bind)."""
        eng = self.engine()
        static, idx, key = self._bind_key(g, prot_x)
        if key != self._batch_key:
            pf = self.__dict__.get("_prefetch")
            if pf is not None:
                self._join_prefetch()
                if pf["key"] == key and prot_x is None:
                    # the batch is bound already -- on the twin handle, by prefetch_graph's worker while the previous step was being
                    # enqueued.  The twin becomes THE engine (everything else keeps reading self._engine); it takes the current
                    # weights with one device-side gather (the optimiser stepped on the other handle since the twin last ran)
                    self._engine, self._twin = self._twin, self._engine
                    eng = self._engine
                    eng.set_flat_params(self._flat)
                    self._batch_key = key
                    self._bound_static = pf["static"]
                    return eng
            eng.set_batch(static[0], g.prot_h, *idx, pocket_uid=g.pocket_uid if prot_x is None else None)
            self._batch_key = key
            self._bound_static = static
        return eng

    @staticmethod
    def _bind_key(g: PocketGraph, prot_x=None):
        static = (g.prot_x if prot_x is None else prot_x, g.prot_h, g.pp_src, g.pp_dst)
        idx = g.index_arrays_i32()
        key = (tuple((t.data_ptr(), t._version, tuple(t.shape), str(t.device)) for t in static),
               idx[0].tobytes(), idx[1].tobytes(),
               None if g.pocket_uid is None else tuple(g.pocket_uid.tolist()))
        return static, idx, key

    def prefetch_graph(self, g: PocketGraph) -> None:
        """Training loops that know their NEXT batch: bind it now, on a second handle (the "twin": own workspace, same weights),
        from a worker thread -- pf_set_pocket_batch is half a step's host time (the pass over 0.65 M pp edges at 256 pockets, the
        index tables, the staging copy: ~0.5 ms), and a training step costs the host as much as the device.  Call it once the
        current step's forward has been issued; the worker's C call runs (GIL released) while this thread enqueues the backward
        and the optimiser step, and the next bind_graph(g) adopts the twin instead of binding.  Both handles enqueue on the
        caller's stream, so the device sees the same order of work as without it; results are those of the single-handle loop
        bit for bit (tests/test_gpu_train.py).  Optional: without the call nothing changes."""
        import threading
        g = as_pocket_graph(g)
        self.engine()
        self._join_prefetch()
        static, idx, key = self._bind_key(g)
        if key == self._batch_key:
            return
        twin = self.__dict__.get("_twin")
        if twin is None or twin.device != self._engine.device:
            twin = PfEngine(device=self._engine.device, **self._arch)
            twin.load_state_dict({k: v for k, v in self.state_dict().items()}, prefix="")
            twin.set_train_precision(getattr(self, "train_precision", "f32"))
            twin.set_train_family(getattr(self, "train_family", "tuned"))
            twin.set_train_input_grads(getattr(self, "train_input_grads", False))
            self.__dict__["_twin"] = twin
        stream = torch.cuda.current_stream(twin.device)
        pf = {"key": key, "static": static, "err": None}

        def work():
            try:
                with torch.cuda.stream(stream):
                    twin.set_batch(static[0], g.prot_h, *idx, pocket_uid=g.pocket_uid)
            except BaseException as e:          # noqa: BLE001  (re-raised by the thread that joins)
                pf["err"] = e
        pf["thread"] = threading.Thread(target=work, name="pfdyn-prefetch", daemon=True)
        self.__dict__["_prefetch"] = pf
        pf["thread"].start()

    def _join_prefetch(self):
        pf = self.__dict__.get("_prefetch")
        if pf is None:
            return
        pf["thread"].join()
        self.__dict__["_prefetch"] = None
        if pf["err"] is not None:
            raise pf["err"]

    def forward(self, g, timestep: torch.Tensor, batch_idxs: Dict[str, torch.Tensor] = None):
        """(eps_h, eps_x) = dynamics(g, t): reads g.x_t, g.h_t (pharm) and g.prot_x, like the reference
        reads g.nodes['pharm'].data['x_t'/'h_t'] and g.nodes['prot'].data['x_0'] (dynamics_gvp.py:139-170)."""
        g = as_pocket_graph(g)
        return self.run(g, g.x_t, g.h_t, timestep, g.prot_x)

    def run(self, g: PocketGraph, x_t, h_t, timestep, prot_x):
        """The boundary call on explicit state tensors.  With autograd enabled and trainable parameters the result
        carries a graph whose backward runs the HIP gradient kernels; in train() mode GVPDropout is applied inside the
        kernels (its seed is drawn from torch's generator, so torch.manual_seed reproduces a step).  Otherwise
        (torch.no_grad() / frozen parameters) the pruned inference path runs."""
        eng = self.bind_graph(g)
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p, _, _ in self._flat_views)
        if not need_grad and not (self.training and self.dropout_rate > 0):
            return eng.dynamics(x_t, h_t, timestep, prot_x=prot_x)
        p_drop = float(self.dropout_rate) if self.training else 0.0
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if p_drop > 0 else 0
        if not need_grad:
            return eng.train_forward(x_t, h_t, timestep, prot_x=prot_x, dropout=p_drop, seed=seed)
        return _DynamicsFn.apply(self, eng, x_t, h_t, timestep, prot_x, p_drop, seed, self.__dict__["_flat_leaf"])


def flat_to_named(flat, layout, shapes):
    """{name: tensor} from a flat vector: ``layout`` = [(name, offset, numel)] (PfEngine.param_layout order), ``shapes`` = {name:
    shape}.  Each tensor is a copy."""
    return {name: flat[off:off + n].reshape(tuple(shapes[name])).clone() for name, off, n in layout}


class FlatAdam:
    """Adam over a PharmRecDynamicsGVP as ONE fused HIP kernel on the flat parameter vector (pf_adam_step) instead of
    a multi-tensor update over 244 tensors: same update rule as torch.optim.Adam(lr, betas, eps, weight_decay)
    (pharmacodiff.py:253).  Uses the flat gradient of the last backward (or of allreduce_gradients).

    The guarded step (pf_adam_step_guarded) is taken when any of ``clip_norm`` (torch.nn.utils.clip_grad_norm_'s max_norm),
    ``clip_value`` (clip_grad_value_; the two exclude each other, as in Lightning), ``ema_decay`` is given, or when ``step`` gets a
    ``grad_scale`` other than 1 (a gradient accumulated over N micro-batches: 1 / N); from then on the optimiser stays on it.
    It norms the whole gradient on the device, SKIPS a step whose gradient holds an inf or NaN (parameters, moments and EMA keep
    their bits; the bias corrections count applied steps only) and keeps ``ema``, a flat exponential moving average of the
    parameters that starts from them at the first guarded step (``ema_warmup``: decay min(d, (1 + k) / (10 + k)) at call k).
    None of this synchronises the host; the counters and the last norm live in a device block that last_grad_norm(),
    last_clip_coef(), skipped_steps() and applied_steps() read -- those four DO synchronise.  Without any of the new arguments
    the class runs pf_adam_step as before, bit for bit."""

    def __init__(self, dynamics: "PharmRecDynamicsGVP", lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 clip_norm=None, clip_value=None, ema_decay=None, ema_warmup=False):
        self.dyn, self.lr, self.betas, self.eps, self.weight_decay = dynamics, lr, betas, eps, weight_decay
        self.t = 0
        self.exp_avg = self.exp_avg_sq = None
        self.param_groups = [{'lr': lr}]            # what LR schedulers / loggers look at
        self._set_options(clip_norm, clip_value, ema_decay, ema_warmup)
        self.ema = None                             # flat EMA of the parameters (guarded step with ema_decay)
        self._state = None                          # the guarded step's device block (PfEngine.optim_state)
        self._calls = 0                             # step() calls on the guarded path, skipped ones included (ema_warmup's k)

    def _set_options(self, clip_norm, clip_value, ema_decay, ema_warmup):
        if clip_norm is not None and clip_value is not None:
            raise ValueError("FlatAdam: clip_norm and clip_value are mutually exclusive (gradient_clip_algorithm is 'norm' OR 'value')")
        for name, v in (("clip_norm", clip_norm), ("clip_value", clip_value)):
            if v is not None and not (float(v) >= 0 and math.isfinite(float(v))):
                raise ValueError(f"FlatAdam: {name} must be a finite number >= 0, got {v!r}")
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"FlatAdam: ema_decay must be in [0, 1), got {ema_decay!r}")
        self.clip_norm = None if clip_norm is None else float(clip_norm)
        self.clip_value = None if clip_value is None else float(clip_value)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)

    @property
    def guarded(self) -> bool:
        return self._state is not None or self.clip_norm is not None or self.clip_value is not None or self.ema_decay is not None

    def _ensure_guard_state(self, eng):
        if self._state is None:
            self._state = eng.optim_state(self.t)
        if self.ema_decay is not None and self.ema is None:
            self.ema = self.dyn._flat.detach().clone()

    def _read_state(self):
        return None if self._state is None else PfEngine.read_optim_state(self._state)

    def applied_steps(self) -> int:
        """Optimiser steps that were applied (skipped ones not counted).  Reads the device block: SYNCHRONISES."""
        st = self._read_state()
        return self.t if st is None else int(st["applied"])

    def skipped_steps(self) -> int:
        """Steps skipped for a non-finite gradient since this object (or its state on a resume) was set up.  SYNCHRONISES."""
        st = self._read_state()
        return 0 if st is None else int(st["skipped"])

    def last_grad_norm(self):
        """Norm of the last guarded step's gradient after grad_scale, before clipping (inf / nan when it was skipped); None
        before the first guarded step.  SYNCHRONISES."""
        st = self._read_state()
        return None if st is None else float(st["norm"])

    def last_clip_coef(self):
        """The factor the last guarded step put on the gradient (1 without norm clipping, 0 when it was skipped).  SYNCHRONISES."""
        st = self._read_state()
        return None if st is None else float(st["coef"])

    def ema_decay_at(self, k: int) -> float:
        d = self.ema_decay or 0.0
        return min(d, (1.0 + k) / (10.0 + k)) if self.ema_warmup else d

    def ema_state_dict(self):
        """The EMA weights as named tensors (state-dict keys of the model, 'dynamics.' prefix; on the host), or None without
        ema_decay.  Before the first guarded step the EMA is the parameters."""
        if self.ema_decay is None:
            return None
        self.dyn.engine()
        flat = self.dyn._flat if self.ema is None else self.ema
        return flat_to_named(flat.detach().cpu(), [("dynamics." + k, off, n) for (k, _), (_, off, n)
                                                   in zip(self.dyn._named_views(), self.dyn._flat_views)],
                             {"dynamics." + k: p.shape for k, p in self.dyn._named_views()})

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context the model runs on the EMA weights (validation, sampling): they are swapped into the flat parameter
        vector and the engine is refreshed; on exit -- also on an exception -- the training weights are back bit for bit.  No
        optimiser step and no backward of an earlier forward inside it."""
        if self.ema_decay is None:
            raise RuntimeError("FlatAdam.ema_weights(): this optimiser keeps no EMA (ema_decay is None)")
        dyn = self.dyn
        dyn.engine()
        if self.ema is None:                        # no guarded step yet: the EMA is the parameters
            yield
            return
        keep = dyn._flat.detach().clone()

        def put(src):
            dyn._join_prefetch()
            with torch.no_grad():
                dyn._flat.copy_(src)
            dyn._engine.set_flat_params(dyn._flat)
            dyn._weights_stamp = dyn._stamp()
            for ent in dyn.__dict__.get("_lane_engines", {}).values():
                ent[1] = None                       # further sampling lanes re-read the flat vector
        put(self.ema)
        try:
            yield
        finally:
            put(keep)

    def zero_grad(self, set_to_none: bool = False, lazy: bool = False):
        """Default (``set_to_none=False``): the flat gradient is zeroed IN PLACE -- one small kernel; the 244 parameters'
        ``.grad`` stay the views of it that the last backward bound, the next backward accumulates into it.  Clearing and
        re-creating 244 views per step costs ~0.8 ms of host time, which is what bounds a step that binds a new batch.
        ``set_to_none=True`` drops everything, like torch.optim's default.
        ``lazy=True`` (training loops that call zero_grad -> backward -> step): nothing is launched here; the next backward of
        the fused loss stores its gradient straight into the bound flat vector (clear and accumulation in one); any other
        gradient -- through the flat leaf or straight into a parameter (a regulariser on p) -- performs the deferred clear
        first, in whichever order a backward delivers them.  Until then ``.grad`` still shows the previous step's values."""
        views = self.dyn._flat_views
        leaf = self.dyn.__dict__.get("_flat_leaf")
        if not set_to_none and leaf is not None and leaf.grad is not None and views:
            p0, o0 = next(((p, o) for p, o, _ in views if p.requires_grad), (None, 0))
            if p0 is not None and p0.grad is not None and p0.grad.data_ptr() == leaf.grad.data_ptr() + 4 * o0:
                if lazy:
                    self.dyn.__dict__["_grad_lazy_zero"] = True
                    self.dyn._last_flat_grad = None         # step() without a backward in between has no gradient
                else:
                    self.dyn.__dict__["_grad_lazy_zero"] = False
                    leaf.grad.zero_()
                return
        self.dyn.__dict__["_grad_lazy_zero"] = False
        for p in ([p for p, _, _ in views] if views else self.dyn.parameters()):
            p.grad = None
        if leaf is not None:
            leaf.grad = None
        self.dyn._last_flat_grad = None

    # -- state: what torch.optim.Adam.state_dict() carries, on the flat vector (checkpoint / resume, rank-0 broadcast) --
    def ensure_state(self, t: int = None, lr: float = None):
        self.dyn.engine()
        if self.exp_avg is None:
            self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.dyn._flat), torch.zeros_like(self.dyn._flat)
        if t is not None:
            self.t = int(t)
            if self._state is not None:             # the device block counts from the given step (skipped starts at 0)
                self._state = self.dyn._engine.optim_state(self.t)
        if lr is not None:
            self.param_groups[0]['lr'] = float(lr)

    def state_dict_meta(self):
        return self.applied_steps(), self.param_groups[0]['lr']

    def state_dict(self):
        """'step' is the APPLIED step count (on the guarded path it is read from the device: synchronises)."""
        self.ensure_state()
        sd = {'state': {'step': self.applied_steps(), 'exp_avg': self.exp_avg.detach().cpu(), 'exp_avg_sq': self.exp_avg_sq.detach().cpu()},
              'param_groups': [{'lr': self.param_groups[0]['lr'], 'betas': self.betas, 'eps': self.eps,
                                'weight_decay': self.weight_decay}],
              'layout': 'flat vector in pf_param_layout order'}
        if self.guarded:
            sd['guard'] = {'clip_norm': self.clip_norm, 'clip_value': self.clip_value, 'ema_decay': self.ema_decay,
                           'ema_warmup': self.ema_warmup, 'calls': self._calls, 'skipped': self.skipped_steps()}
            if self.ema is not None:
                sd['state']['ema'] = self.ema.detach().cpu()
        return sd

    def load_state_dict(self, sd):
        """Accepts this class's own state (flat moment vectors, marked by 'layout') and the per-parameter state of
        torch.optim.Adam -- what a checkpoint written by the reference's Lightning run holds (pharmacodiff.py:253-263:
        Adam(self.parameters())): parameter i of that optimiser is tensor i of the flat layout (state-dict order, the
        empty dummy_param included); parameters without an entry (never stepped) keep zero moments."""
        st, pg = sd['state'], sd['param_groups'][0]
        self.ema = None                             # states without an EMA vector: it starts from the parameters
        if 'layout' in sd:
            self.ensure_state(st['step'], pg['lr'])
            if st['exp_avg'].numel() != self.exp_avg.numel():
                raise ValueError("FlatAdam.load_state_dict: moment vectors do not match this model's parameter count")
            self.exp_avg.copy_(st['exp_avg'])
            self.exp_avg_sq.copy_(st['exp_avg_sq'])
            guard = sd.get('guard')
            if guard is not None:                   # the state's options replace the constructor's; the step count goes to the device
                self._set_options(guard.get('clip_norm'), guard.get('clip_value'), guard.get('ema_decay'), guard.get('ema_warmup', False))
                self._calls = int(guard.get('calls', st['step']))
                if st.get('ema') is not None and self.ema_decay is not None:
                    if st['ema'].numel() != self.exp_avg.numel():
                        raise ValueError("FlatAdam.load_state_dict: the EMA vector does not match this model's parameter count")
                    self.ema = st['ema'].to(self.exp_avg.device, torch.float32).clone()
        else:
            # parameter i of that optimiser = the i-th entry of the model's parameters(): PharmacophoreDiff's list is
            # gamma.gamma (a frozen nn.Parameter upstream, pharmacodiff.py:662-664: never stepped) followed by the dynamics
            # module's parameters in registration order, the empty dummy_param tensors included; an optimiser built on
            # model.dynamics.parameters() lacks the leading gamma
            where = {name: (off, n) for name, off, n in self.dyn.engine().param_layout()}
            names = ['dynamics.' + k for k, _ in self.dyn.named_parameters()]
            ids = list(pg.get('params', range(len(names))))
            if len(ids) == len(names) + 1:
                names = ['gamma.gamma'] + names
            elif len(ids) != len(names):
                raise ValueError(f"FlatAdam.load_state_dict: the optimiser state names {len(ids)} parameters, this model has "
                                 f"{len(names)} (+ gamma.gamma)")
            steps = [int(torch.as_tensor(st[i]['step']).item()) for i in ids if i in st and 'step' in st[i]]
            self.ensure_state(max(steps) if steps else 0, pg['lr'])
            self.exp_avg.zero_(); self.exp_avg_sq.zero_()
            for i, name in zip(ids, names):
                if i not in st or name not in where or where[name][1] == 0:
                    continue
                off, n = where[name]
                for key, dst in (('exp_avg', self.exp_avg), ('exp_avg_sq', self.exp_avg_sq)):
                    src = st[i][key].reshape(-1)
                    if src.numel() != n:
                        raise ValueError(f"FlatAdam.load_state_dict: moment of {name} has {src.numel()} elements, expected {n}")
                    dst[off:off + n].copy_(src)
        self.betas, self.eps = tuple(pg.get('betas', self.betas)), pg.get('eps', self.eps)
        self.weight_decay = pg.get('weight_decay', self.weight_decay)

    def step(self, grad_scale: float = 1.0):
        """One optimiser step on the flat gradient times ``grad_scale`` (1 / N after N accumulated micro-batches)."""
        dyn = self.dyn
        g = getattr(dyn, "_last_flat_grad", None)
        if g is None:
            raise RuntimeError("FlatAdam.step(): no gradient (run loss.backward() on a training forward first)")
        # the engine that produced this gradient (the forward's bind checked the parameter views and synchronised it; another
        # pass over the 244 parameters here is 0.1 ms of a 1.6 ms step); engine() only when there is none yet
        # Cheap guard on that fast path: parameters re-materialised between backward() and step() (module.to(),
        # an assignment to p.data) no longer view the flat vector; the first and the last view are checked every step,
        # all of them every 64th, and a mismatch falls back to engine(), which re-homes and re-synchronises them.
        fast = dyn._engine is not None and dyn._flat is not None and dyn._flat.is_cuda and bool(dyn._flat_views)
        if fast:
            base = dyn._flat.data_ptr()
            ends = (dyn._flat_views[0], dyn._flat_views[-1])
            tick = self._calls if self._state is not None else self.t
            fast = all(p.data_ptr() == base + 4 * off for p, off, _ in ends) and (tick % 64 != 63 or dyn._views_intact())
        if not fast:
            eng = dyn.engine()
            if g.numel() != dyn._flat.numel() or g.device != dyn._flat.device:
                raise RuntimeError("FlatAdam.step(): the parameters were re-allocated after backward(); run the step's "
                                   "forward and backward again")
        else:
            eng = dyn._engine
        if self.exp_avg is None:
            self.exp_avg, self.exp_avg_sq = torch.zeros_like(dyn._flat), torch.zeros_like(dyn._flat)
        if self.guarded or float(grad_scale) != 1.0:
            # clipping, the non-finite skip, the EMA stream and the scale in the library's three launches; the applied step count
            # stays on the device (self.t is not advanced: applied_steps() reads it)
            self._ensure_guard_state(eng)
            eng.adam_step_guarded(dyn._flat, g, self.exp_avg, self.exp_avg_sq, self._state, self.param_groups[0]['lr'], self.betas,
                                  self.eps, self.weight_decay, grad_scale=grad_scale, clip_norm=self.clip_norm,
                                  clip_value=self.clip_value, ema=self.ema, ema_decay=self.ema_decay_at(self._calls))
            self._calls += 1
            return
        self.t += 1
        eng.adam_step(dyn._flat, g, self.exp_avg, self.exp_avg_sq, self.t, self.param_groups[0]['lr'], self.betas, self.eps,
                      self.weight_decay)
        # the engine already holds the new values (its kernel wrote the flat vector the parameter views share) and the kernel does not
        # touch the views' version counters: the stamp engine() took for this step still describes them.  (Re-reading the 244
        # counters here was 40 us of host time per step; a parameter modified in place between the forward and this call makes the
        # next engine() upload the flat vector once more, which is correct either way.)



def screen_library(queries, library, engine: Optional[PfEngine] = None, top_k: int = 10, min_match: float = 0.0, sigma: float = 1.0,
                   tolerance: float = 1.5, refine: int = 4, min_area: float = 1.0, max_pairs: int = ALIGN_MAX_PAIRS) -> List[List[ScreenHit]]:
    """One list of ScreenHit per query, best first: every library entry is superposed onto every query, the entries
    with n_matched >= ceil(min_match * n_q) qualify, and the ``top_k`` of them by (sim descending, entry index) are returned.
    ``queries``: samples, ConsensusPharmacophore objects or (x, types) pairs of at most 16 centers (ValueError above);
    ``library``: a PharmacophoreLibrary (or a list of entries).  With an ``engine`` the pairs are computed on its device
    (PfEngine.align, pf_pharm_align), the library uploaded once; without one by analysis.align_pharmacophores on the host, same
    definition.  Either way the work is cut into calls of at most ``max_pairs`` (the call's cap, 2^24) pairs."""
    opts = dict(zip(("sigma", "tolerance", "refine", "min_area"), _align_options(sigma, tolerance, refine, min_area)))
    qs = _align_queries(queries)
    lib = library if isinstance(library, PharmacophoreLibrary) else PharmacophoreLibrary(library)
    if not 0.0 <= float(min_match) <= 1.0:
        raise ValueError("min_match must be in [0, 1]")
    max_pairs = int(max_pairs)
    if not 1 <= max_pairs <= ALIGN_MAX_PAIRS:
        raise ValueError(f"max_pairs must be in [1, {ALIGN_MAX_PAIRS}]")
    Q, L = len(qs), len(lib)
    if Q == 0 or L == 0:
        return [[] for _ in range(Q)]
    sim, matched = torch.zeros(Q, L), torch.zeros(Q, L, dtype=torch.int64)
    xf = torch.zeros(Q, L, 12)
    q_step = min(Q, max_pairs)
    l_step = max(1, max_pairs // q_step)
    if engine is not None:
        lx, lt, lptr = lib.packed()
        lx, lt = lx.to(engine.device, torch.float32), lt.to(engine.device, torch.int32)
    for q0 in range(0, Q, q_step):
        qc = qs[q0:q0 + q_step]
        for l0 in range(0, L, l_step):
            l1 = min(l0 + l_step, L)
            if engine is None:
                r = align_pharmacophores(qc, lib.entries[l0:l1], **opts)
            else:
                qptr = np.concatenate([[0], np.cumsum([x.shape[0] for x, _ in qc])]).astype(np.int32)
                c0, c1 = int(lptr[l0]), int(lptr[l1])
                r = engine.align(torch.cat([x for x, _ in qc]), torch.cat([t for _, t in qc]), qptr, lx[c0:c1], lt[c0:c1],
                                 (lptr[l0:l1 + 1] - lptr[l0]).numpy(), **opts)
            sim[q0:q0 + len(qc), l0:l1] = r["sim"].cpu().float()
            matched[q0:q0 + len(qc), l0:l1] = r["n_matched"].cpu().long()
            xf[q0:q0 + len(qc), l0:l1] = r["transform"].cpu().float()
    out = []
    for a, (x, _) in enumerate(qs):
        need = math.ceil(float(min_match) * x.shape[0] - 1e-9)
        ok = [b for b in range(L) if int(matched[a, b]) >= need]
        ok.sort(key=lambda b: (-float(sim[a, b]), b))
        out.append([ScreenHit(b, lib.names[b], sim[a, b], matched[a, b], xf[a, b], lib[b]) for b in ok[:int(top_k)]])
    return out


def sample_sets(per_pocket_samples, engine: Optional[PfEngine] = None, sigma: float = 1.0, tolerance: float = 1.5,
                threshold: float = 0.5, min_support: float = 0.5) -> List[Optional[SampleSet]]:
    """One SampleSet per pocket (None for a pocket without samples) from per-pocket lists of SampledPharmacophore objects or
    (x [n, 3], type indices [n]) pairs, each pocket's samples in that pocket's frame.  With an ``engine`` the sets are analysed
    on its device (PfEngine.sample_set, pf_sample_set_analyze): many pockets per call, a new call whenever the similarity
    matrices of the next pocket would take the call over its cap of 2^26 floats.  Without one: analysis.analyze_sample_set on
    the host, same definitions."""
    sigma, tolerance, threshold = _sset_options(sigma, tolerance, threshold)
    opts = dict(sigma=sigma, tolerance=tolerance, threshold=threshold, min_support=float(min_support))
    pockets = [_sset_samples(ps) if len(ps) else None for ps in per_pocket_samples]
    out: List[Optional[SampleSet]] = [None] * len(pockets)
    if engine is None:
        for r, ps in enumerate(pockets):
            if ps is not None:
                out[r] = analyze_sample_set(ps, **opts)
        return out
    chunk, floats = [], 0

    def flush():
        if not chunk:
            return
        samples = [s for r in chunk for s in pockets[r]]
        set_ptr = np.concatenate([[0], np.cumsum([len(pockets[r]) for r in chunk])]).astype(np.int32)
        center_ptr = np.concatenate([[0], np.cumsum([s[0].shape[0] for s in samples])]).astype(np.int32)
        res = engine.sample_set(torch.cat([s[0] for s in samples]), torch.cat([s[1] for s in samples]), set_ptr, center_ptr,
                                sigma=sigma, tolerance=tolerance, threshold=threshold)
        res = {k: v.cpu() for k, v in res.items()}
        at = 0
        for p, r in enumerate(chunk):
            s0, s1 = int(set_ptr[p]), int(set_ptr[p + 1])
            S, k = s1 - s0, int(res["n_clusters"][p])
            rows = lambda a: slice(int(center_ptr[s0 + a]), int(center_ptr[s0 + a + 1]))
            centroids = res["centroid"][s0:s0 + k].tolist()
            cons = [(res["cons_x"][rows(m)], pockets[r][m][1], res["cons_cnt"][rows(m)]) for m in centroids]
            out[r] = SampleSet(res["similarity"][at:at + S * S].reshape(S, S), [res["support"][rows(a)] for a in range(S)],
                               res["label"][s0:s1], centroids, cons, None, opts)
            at += S * S
        chunk.clear()

    for r, ps in enumerate(pockets):
        if ps is None:
            continue
        if floats + len(ps) ** 2 > SSET_MAX_SIM:
            flush()
            floats = 0
        chunk.append(r)
        floats += len(ps) ** 2
    flush()
    return out


class PharmSizeDistribution:
    """pharmacoforge/models/n_nodes_dist.py:7-14 (sample_uniformly only; sample_variety is broken upstream)."""

    def __init__(self, dataset_dir=None):
        pass

    def sample_uniformly(self, n_replicates) -> torch.Tensor:
        return torch.from_numpy(np.random.randint(3, 9, n_replicates))


# ---------------------------------------------------------------------------------------------
@dataclasses.dataclass
class PocketField:
    """Pocket-derived guidance of a sampling run (PharmacophoreDiff.sample(pocket_field=...); the energies: include/pfdyn.h,
    "pocket field").  ``clash_radius``: None (no clash term), a float for every atom, or a per-atom tensor ([n_atoms] of the pocket;
    for several pockets a list with one entry per pocket) -- a center of the predicted clean sample inside that radius of an atom
    is pushed out with ``clash_weight``; a radius of 0 makes an atom inert.  ``comp_weight`` > 0: a center of type t is pulled to
    within the matching distance of a complementary receptor feature (the graph's prot_ph_x / prot_ph_h; the table and the
    distances are analysis._MATCHING_TYPES / _MATCHING_DIST, what SampleAnalyzer's validity counts); ``kappa`` (1 / angstrom) is
    the sharpness of the soft minimum over the matching features, ``type_sharpness`` that of the soft type assignment, on
    one-hot-scaled features (the model multiplies it by its pharm_feat_norm_constant)."""
    clash_radius: object = 2.0
    clash_weight: float = 1.0
    comp_weight: float = 0.0
    kappa: float = 4.0
    type_sharpness: float = 4.0


@dataclasses.dataclass
class TypeGuidance:
    """Guidance of the centers' feature rows in a guided run (PharmacophoreDiff.sample(type_restraints=..., type_guidance=...);
    the semantics: include/pfdyn.h, "type guidance").  ``scale``: the feature shift's scale (0: the rows stay where the run
    without it puts them); ``clip`` > 0: a row's shift is clipped to that Euclidean norm; ``sharpness``: that of the soft type
    assignment, on one-hot-scaled features (the model multiplies it by its pharm_feat_norm_constant) -- None: the pocket field's
    when there is one, else 4; with a pocket field the two must agree.  ``complementarity``: the pocket field's complementarity
    energy steers the types as well (it needs a PocketField with comp_weight > 0); a type without any partner in the pocket then
    costs ``unmatched``^2 per unit of comp_weight."""
    scale: float = 1.0
    clip: float = 0.0
    sharpness: Optional[float] = None
    complementarity: bool = False
    unmatched: float = 0.0


@dataclasses.dataclass(frozen=True)
class RunSpec:
    """What the keywords of sample / sample_given_receptor ask for, resolved and checked once per call
    (PharmacophoreDiff._run_spec applies every composition rule); host values only.  ``top``: the level the run starts at, T or
    a seeded run's seed level.  ``fewstep``: None or (N, sampler, eta, spacing) (_fewstep).  ``guided``: restraints or a pocket
    field are present somewhere in the call.  What a single batch runs follows from it and two facts of the batch: batch()."""
    T: int
    top: int
    seeded: bool
    fewstep: Optional[tuple]
    pin_resamples: int
    pin_jump: int
    guide_scale: float
    guide_clip: float
    guide_family: str
    guided: bool
    types: Optional[tuple] = None               # None, or types_next's scalars (scale, clip, sharpness, complementarity, unmatched)
    separation: Optional[tuple] = None          # None, or (d, w) of min_separation: the pair restraint (*, *, d, inf, w) on every graph

    def pairs_arg(self, pair_restraints, n_graphs):
        """PfEngine.pairs_next's argument of a guided batch: its graphs' pair restraints (None or one list or None per graph) with
        the minimum separation's row appended to every graph; None: the call has neither"""
        if pair_restraints is None and self.separation is None:
            return None
        rows = [list(r or []) for r in (pair_restraints if pair_restraints is not None else [None] * n_graphs)]
        if self.separation is not None:
            d, w = self.separation
            rows = [r + [(None, None, d, math.inf, w)] for r in rows]
        return [r or None for r in rows]

    def types_kwargs(self, type_restraints):
        """PfEngine.types_next's arguments of a guided batch (None: the call has no type guidance)"""
        if self.types is None:
            return None
        scale, clip, sharp, comp, unmatched = self.types
        return dict(restraints=type_restraints, scale=scale, clip=clip, sharpness=sharp, complementarity=comp, unmatched=unmatched)

    def batch(self, m, has_pins, guided):
        """One batch's run, given whether a pin flag is set in it and whether it is guided (a restraint in it, or a pocket field):
        (kind, n_ops, noise rows, coef_arr, the further array keywords of PfEngine.sample).  kind: 'multistep' (pf_sample_ms; 1
        row, the initial draw), 'resampled' (a flag and pin_resamples > 1: pf_sample_pinned_resampled over
        schedule.resample_plan(top, jump, resamples)), else 'guided', 'pinned' or 'plain'; these visit top (few-step: N) levels
        and read one row more.  The arrays are the model's cached ones (``m``: _step_arrays, _fewstep_arrays, _plan_arrays)."""
        few, top = self.fewstep, self.top
        arrays = m._step_arrays if few is None else (lambda name, top: m._fewstep_arrays(name, few, top))
        n_ops = top if few is None else few[0]
        if few is not None and few[1] == "multistep":
            return "multistep", n_ops, 1, None, {"ms_coef_arr": arrays("ms", top)}
        if has_pins and self.pin_resamples > 1:
            n_ops, arr, parr, op_arr, re_arr = m._plan_arrays(self.pin_jump, self.pin_resamples, top)
            return "resampled", n_ops, n_ops + 1, arr, {"pin_coef_arr": parr, "plan": (op_arr, re_arr)}
        kw = {"pin_coef_arr": arrays("pin", top)} if guided or has_pins else {}
        if guided:
            kw.update(guide_coef_arr=arrays("guide", top), guide_scale=self.guide_scale, guide_clip=self.guide_clip,
                      guide_family=self.guide_family)
        return "guided" if guided else "pinned" if has_pins else "plain", n_ops, n_ops + 1, arrays("coef", top), kw


class PharmacophoreDiff(_Base):
    """Drop-in for pharmacoforge.models.pharmacodiff.PharmacophoreDiff on the sampling / evaluation
    path.  Constructor arguments, attribute names, state-dict keys ('gamma.gamma', 'dynamics.*') and
    the metric names follow the reference (pharmacodiff.py:27-78, 231-239)."""

    def __init__(self, pharm_nf, rec_nf, ph_type_map: List[str], processed_data_dir: Path = None,
                 n_timesteps: int = 1000, graph_config={}, dynamics_config={}, lr_scheduler_config={},
                 sample_interval: float = 1, val_loss_interval: float = 1, batch_size: int = 64,
                 pharms_per_pocket: int = 8, n_pockets_to_sample: int = 8, precision=1e-4,
                 pharm_feat_norm_constant=1, endpoint_param_feat: bool = False, endpoint_param_coord: bool = False,
                 weighted_loss: bool = False, remove_com: bool = True, **kwargs):
        super().__init__()
        self.n_pharm_feats, self.n_prot_feats = pharm_nf, rec_nf
        self.batch_size = batch_size
        self.ph_type_map = ph_type_map
        self.n_timesteps = n_timesteps
        self.remove_com = remove_com
        self.pharm_feat_norm_constant = pharm_feat_norm_constant
        self.endpoint_param_feat, self.endpoint_param_coord = endpoint_param_feat, endpoint_param_coord
        self.weighted_loss = weighted_loss
        self.pharm_size_dist = PharmSizeDistribution(processed_data_dir)
        self.gamma = PredefinedNoiseSchedule(noise_schedule='polynomial_2', timesteps=n_timesteps, precision=precision)
        self.dynamics = PharmRecDynamicsGVP(pharm_nf, rec_nf, **graph_config, **dynamics_config)
        self.lr_scheduler_config = lr_scheduler_config
        self.sample_interval, self.pharms_per_pocket = sample_interval, pharms_per_pocket
        self.n_pockets_to_sample = n_pockets_to_sample
        self.last_sample_marker = 0
        self.last_epoch_exact = 0
        self.val_loss_interval = val_loss_interval
        self._hparams_dict = dict(pharm_nf=pharm_nf, rec_nf=rec_nf, ph_type_map=ph_type_map,
                                  processed_data_dir=processed_data_dir, n_timesteps=n_timesteps,
                                  graph_config=graph_config, dynamics_config=dynamics_config,
                                  lr_scheduler_config=lr_scheduler_config, sample_interval=sample_interval,
                                  val_loss_interval=val_loss_interval, batch_size=batch_size,
                                  pharms_per_pocket=pharms_per_pocket, n_pockets_to_sample=n_pockets_to_sample,
                                  precision=precision, pharm_feat_norm_constant=pharm_feat_norm_constant,
                                  endpoint_param_feat=endpoint_param_feat, endpoint_param_coord=endpoint_param_coord,
                                  weighted_loss=weighted_loss, remove_com=remove_com, **kwargs)
        if pl is not None:
            self.save_hyperparameters()
        self._coef = None
        self._arrays = {}                       # _host_arrays

    # -- Lightning-free conveniences ----------------------------------------------------------
    if pl is None:
        @property
        def device(self) -> torch.device:
            return next(self.parameters()).device

        @classmethod
        def load_from_checkpoint(cls, checkpoint_path, map_location="cpu", **overrides):
            """A Lightning .ckpt is a torch-loadable dict with 'state_dict' and 'hyper_parameters'."""
            ckpt = torch.load(str(checkpoint_path), map_location=map_location, weights_only=False)
            hp = dict(ckpt.get("hyper_parameters", {}))
            hp.update(overrides)
            model = cls(**hp)
            model.load_state_dict(ckpt["state_dict"], strict=True)
            return model

        def log_dict(self, *a, **k):
            pass

    def save_checkpoint(self, path, ema_state_dict=None, **extra):
        """Write a file ``load_from_checkpoint`` (ours or Lightning's) can read.  ``extra``: further top-level entries in
        Lightning's checkpoint vocabulary ('epoch', 'global_step', 'optimizer_states', 'lr_schedulers').  ``ema_state_dict``
        (FlatAdam.ema_state_dict()): the EMA weights as named tensors, stored under 'ema_state_dict' for load_ema_weights."""
        if ema_state_dict is not None:
            extra = dict(extra, ema_state_dict=ema_state_dict)
        torch.save({"state_dict": self.state_dict(), "hyper_parameters": self._hparams_dict, **extra}, str(path))

    def load_ema_weights(self, path_or_dict):
        """Replace the dynamics' weights with the EMA weights of a checkpoint (a path, a loaded checkpoint dict, or the named
        tensors themselves).  A checkpoint without them raises a KeyError that names the missing key, 'ema_state_dict'."""
        src = path_or_dict
        if not isinstance(src, dict):
            src = torch.load(str(src), map_location="cpu", weights_only=False)
        if "ema_state_dict" in src:
            ema = src["ema_state_dict"]
        elif "state_dict" in src or "hyper_parameters" in src or not src:
            raise KeyError("load_ema_weights: the checkpoint has no 'ema_state_dict' entry (it was written without EMA weights: "
                           "train with ema_decay set)")
        else:
            ema = src
        own = self.state_dict()
        unknown = [k for k in ema if k not in own]
        if unknown:
            raise KeyError(f"load_ema_weights: 'ema_state_dict' names tensors this model does not have: {unknown[:3]}")
        for k, v in ema.items():
            if tuple(v.shape) != tuple(own[k].shape):
                raise ValueError(f"load_ema_weights: {k} has shape {tuple(v.shape)}, the model's is {tuple(own[k].shape)}")
        with torch.no_grad():
            for k, v in ema.items():
                own[k].copy_(v)                     # state_dict() tensors alias the parameters (views of the flat vector on a GPU)
        return self

    # -- small algebra (pharmacodiff.py:80-86, 140-160) ----------------------------------------
    def sigma(self, gamma):
        return _sigma(gamma)

    def alpha(self, gamma):
        return _alpha(gamma)

    def sigma_and_alpha_t_given_s(self, gamma_t, gamma_s):
        return sigma_and_alpha_t_given_s(gamma_t, gamma_s)

    def step_coefficients(self):
        if self._coef is None:
            self._coef = step_coefficients(self.gamma.gamma, self.n_timesteps)
        return self._coef

    # -- sampling (pharmacodiff.py:433-514) ------------------------------------------------------
    @torch.no_grad()
    def sample_given_receptor(self, g, init_pharm_com: torch.Tensor = None, visualize_trajectory: bool = False,
                              noise: torch.Tensor = None, pin_resamples: int = 1, pin_jump: int = 10, restraints=None,
                              guide_scale: float = 1.0, guide_clip: float = 0.0, seeds=None, seed_level: int = None,
                              seed_keep=None, sample_steps: int = None, sampler: str = None, eta: float = None,
                              spacing: str = None, guide_family: str = "wide", pocket_field=None, type_restraints=None,
                              type_guidance=None, pair_restraints=None, min_separation: float = None,
                              separation_weight: float = 1.0) -> List[SampledPharmacophore]:
        """Reverse diffusion for a batch of pocket graphs; the whole T-step loop is enqueued on the
        current HIP stream by pf_sample (no host synchronisation inside the loop).

        ``noise`` ([T+1, Nf, 3+pharm_nf], optional) injects the Gaussian draws (initial draw first; x
        columns before h columns -- the reference's draw order, pharmacodiff.py:455-456, 423-424): replaying a
        reference run means passing its draws here.  When omitted all T+1 draws come from ONE torch.randn call on the
        model's device (same distribution, reproducible under torch.manual_seed; the reference's 2(T+1) separate calls
        would cost a thousand launches per batch and cannot reproduce a CUDA generator's stream on ROCm anyway).

        Pinned centers: when the graph carries ``pharm_pin`` / ``pharm_pin_x`` / ``pharm_pin_h`` with a non-zero flag, the
        run is pf_sample_pinned -- the flagged centers are replaced by the given values at every step's noise level and
        come back bit for bit; the free centers are placed around them.  With ``pin_resamples`` r > 1 such a run is
        pf_sample_pinned_resampled: every stretch of ``pin_jump`` levels is re-noised to its upper level and denoised again,
        r times in all (schedule.resample_plan), so that the free centers can react to the given ones; it has n_ops ~ r T ops
        and ``noise`` must then have n_ops + 1 rows.  A graph batch without a flag set ignores both.

        ``restraints``: None, or one list (or None) per graph of the batch of (kind, center, point, radius, weight) (see
        ``sample``): with a restraint in it the run is pf_sample_guided with ``guide_scale`` / ``guide_clip``, on the kernel
        family ``guide_family`` names ('wide', the default, or 'tuned': see ``sample``).  ``pocket_field`` (a PocketField whose
        per-atom radii, if any, cover the batch's atoms): the run is guided also without restraints (see ``sample``).
        ``type_restraints``: None, or one list (or None) per graph of the batch of (type, center, point, radius, weight), with
        ``type_guidance`` (a TypeGuidance): the run steers the feature rows too (see ``sample``).
        ``pair_restraints``: None, or one list (or None) per graph of the batch of (i, j, lo, hi, weight); ``min_separation`` d
        with ``separation_weight``: (*, *, d, inf, weight) on every graph (see ``sample``).

        ``seeds`` with ``seed_level`` a (and optionally ``seed_keep``): a seeded run (pf_sample_seed_next) -- one (x [n,3], types
        [n]) per graph of the batch, n that graph's number of centers; the run starts from the seeds noised to level a and makes
        the steps a-1 .. 0, so ``noise`` has a + 1 rows (n_ops + 1 with ``pin_resamples`` > 1, whose plan then starts at a).
        ``seed_keep``: per graph, the seed centers that stay fixed in position and type (see ``sample``).

        ``sample_steps`` N with ``sampler`` / ``eta`` / ``spacing``: a few-step run (see ``sample``) -- ``noise`` has N + 1 rows for
        the first-order samplers and 1 row for 'multistep'; trajectories have N + 1 frames."""
        g = as_pocket_graph(g)
        type_restraints = self._type_restraints(type_restraints, g.batch_size, "graphs")
        pair_restraints = self._pair_restraints(pair_restraints, g.batch_size, "graphs",
                                                [[n] for n in (g.pharm_ptr[1:] - g.pharm_ptr[:-1]).tolist()], int(min_separation is not None))
        spec = self._run_spec(pins=self._has_pins(g),
                              guided=self._guided(restraints, pocket_field, type_restraints, pair_restraints, min_separation),
                              pinned=g.pharm_pin is not None,
                              pin_resamples=pin_resamples, pin_jump=pin_jump, guide_scale=guide_scale, guide_clip=guide_clip,
                              seeds=seeds, seed_level=seed_level, seed_keep=seed_keep, sample_steps=sample_steps, sampler=sampler,
                              eta=eta, spacing=spacing, guide_family=guide_family, pocket_field=pocket_field,
                              type_guidance=type_guidance, typed=type_restraints is not None, min_separation=min_separation,
                              separation_weight=separation_weight)
        if seeds is not None:
            sizes = (g.pharm_ptr[1:] - g.pharm_ptr[:-1]).tolist()
            fields = self._seed_fields([[n] for n in sizes], seeds, seed_keep, batch=True)
            g = self._with_pin_fields(g, *(torch.cat(f) for f in zip(*fields)))
        return self._sample_finish(self._sample_fetch(self._sample_enqueue(g, spec, init_pharm_com, visualize_trajectory, noise,
                                                                           restraints=restraints,
                                                                           field=self._field_for_batch(g, pocket_field),
                                                                           type_restraints=type_restraints,
                                                                           pair_restraints=pair_restraints)))

    @staticmethod
    def _has_pins(g):
        """a graph (of one pocket, or batched) carries a pin flag that is set: what makes a run pinned"""
        return g.pharm_pin is not None and bool((g.pharm_pin != 0).any())

    @staticmethod
    def _guided(restraints, field, type_restraints=None, pair_restraints=None, min_separation=None):
        """a pocket field or a minimum separation, or a restraint, type restraint or pair restraint in one of the per-pocket /
        per-graph lists (None or empty: none): what makes a run guided"""
        return (field is not None or min_separation is not None or (restraints is not None and any(restraints))
                or (type_restraints is not None and any(type_restraints)) or (pair_restraints is not None and any(pair_restraints)))

    @staticmethod
    def _pair_restraints(pair_restraints, n, what, sizes=None, extra=0):
        """``pair_restraints`` of sample / sample_given_receptor, checked before any device work: None when there is none, else one
        list or None per pocket / graph of (i or None, j or None, lo, hi, weight).  ``sizes``: per entry the numbers of centers
        asked for; an index that one of them does not have is an error here.  ``extra``: rows the call adds to every graph (a minimum
        separation's), which count towards the library's 256 per graph."""
        if pair_restraints is None:
            return None
        if len(pair_restraints) != n:
            raise ValueError(f"pair_restraints lists {len(pair_restraints)} entries for {n} {what}")
        index = lambda c: None if c is None or c == "*" or int(c) < 0 else int(c)
        out = []
        for r, rs in enumerate(pair_restraints):
            rows = []
            for row in (rs or []):
                if len(row) != 5:
                    raise ValueError(f"a pair restraint is (i, j, lo, hi, weight), got {row!r}")
                i, j, lo, hi, w = index(row[0]), index(row[1]), float(row[2]), float(row[3]), float(row[4])
                if i is not None and i == j:
                    raise ValueError(f"a pair restraint names two different centers, got {i} twice")
                if not (0 <= lo < math.inf and lo <= hi):
                    raise ValueError(f"a pair restraint needs 0 <= lo <= hi with lo finite (hi = inf: no upper bound), got lo {lo}, hi {hi}")
                if not 0 <= w < math.inf:
                    raise ValueError(f"a pair restraint's weight must be finite and >= 0, got {w}")
                for c in (i, j):
                    small = [int(m) for m in (sizes[r] if sizes is not None else []) if c is not None and int(m) <= c]
                    if small:
                        raise ValueError(f"{what[:-1]} {r}: a pair restraint names center {c} but sizes {small} were requested")
                rows.append((i, j, lo, hi, w))
            if len(rows) + extra > 256:
                raise ValueError(f"{what[:-1]} {r}: {len(rows)} pair restraints{' and a minimum separation' if extra else ''} (at most 256 per graph)")
            out.append(rows or None)
        return out if any(out) else None

    def _type_index(self, t):
        """a type restraint's type: an index, or a name of the model's ph_type_map"""
        if isinstance(t, str):
            if t not in self.ph_type_map:
                raise ValueError(f"a type restraint names type {t!r}; this model's types are {list(self.ph_type_map)}")
            return list(self.ph_type_map).index(t)
        t = int(t)
        if not 0 <= t < self.n_pharm_feats:
            raise ValueError(f"a type restraint's type index must be in 0..{self.n_pharm_feats - 1}, got {t}")
        return t

    def _type_restraints(self, type_restraints, n, what):
        """``type_restraints`` of sample / sample_given_receptor, checked before any device work: None when there is none, else one
        list or None per pocket / graph of (type index, center or None, point, radius, weight)"""
        if type_restraints is None:
            return None
        if len(type_restraints) != n:
            raise ValueError(f"type_restraints lists {len(type_restraints)} entries for {n} {what}")
        out = []
        for rs in type_restraints:
            rows = []
            for row in (rs or []):
                if len(row) != 5:
                    raise ValueError(f"a type restraint is (type, center, point, radius, weight), got {row!r}")
                t, c, p, r, w = row
                rows.append((self._type_index(t), None if c is None or c == "*" or int(c) < 0 else int(c), tuple(float(v) for v in p),
                             float(r), float(w)))
            out.append(rows or None)
        return out if any(out) else None

    @staticmethod
    def _with_pin_fields(g, flags, x, h):
        dev = g.prot_x.device
        return dataclasses.replace(g, pharm_pin=flags.to(dev), pharm_pin_x=x.to(dev), pharm_pin_h=h.to(dev))

    def _run_spec(self, pins, guided, pinned=False, pin_resamples=1, pin_jump=10, guide_scale=1.0, guide_clip=0.0, seeds=None,
                  seed_level=None, seed_keep=None, score_levels=None, sample_steps=None, sampler=None, eta=None, spacing=None,
                  guide_family="wide", pocket_field=None, type_guidance=None, typed=False, min_separation=None, separation_weight=1.0):
        """The RunSpec of one sample / sample_given_receptor call from its keywords; every rule on how they compose is applied
        here, once, before any device work.  The two callers differ in where they look: ``pins`` -- a pin is present (an entry of
        ``pinned``; a flag set on the batched graph), ``guided`` (_guided), ``pinned`` -- pin fields were given at all.  ``typed``: a type
        restraint is present; ``type_guidance``: None or a TypeGuidance (``typed`` alone means TypeGuidance()); ``pocket_field``:
        the call's, for the rules that tie the two.  ``min_separation`` d with ``separation_weight`` w: the pair restraint
        (*, *, d, inf, w) on every graph, which makes every batch guided (the callers' ``guided`` says so: _guided)."""
        if score_levels is not None and not 1 <= int(score_levels) <= self.n_timesteps:
            raise ValueError(f"score_levels must satisfy 1 <= K <= {self.n_timesteps}, got {score_levels}")
        self._check_guide_family(guide_family)
        fewstep = self._fewstep(sample_steps, sampler, eta, spacing, pin_resamples=pin_resamples, seed_level=seed_level,
                                pins=pins or seed_keep is not None, restraints=guided)
        if pin_resamples < 1 or pin_jump < 1:
            raise ValueError(f"pin_resamples and pin_jump must be at least 1, got {pin_resamples} and {pin_jump}")
        if guided and pin_resamples > 1:
            raise ValueError("restraints together with pin_resamples > 1: guidance with resampling jumps is not supported")
        types = None
        if type_guidance is not None or typed:
            tg = TypeGuidance() if type_guidance is None else type_guidance
            if not isinstance(tg, TypeGuidance):
                raise ValueError(f"type_guidance must be a TypeGuidance, got {type(tg).__name__}")
            field_sharp = None if pocket_field is None else float(getattr(pocket_field, "type_sharpness", 4.0))
            sharp = float(tg.sharpness) if tg.sharpness is not None else 4.0 if field_sharp is None else field_sharp
            if field_sharp is not None and sharp != field_sharp:
                raise ValueError(f"type_guidance.sharpness ({sharp}) and pocket_field.type_sharpness ({field_sharp}) must agree")
            if tg.complementarity and not (pocket_field is not None and float(getattr(pocket_field, "comp_weight", 0.0)) > 0):
                raise ValueError("type_guidance.complementarity needs a pocket_field with comp_weight > 0")
            for name in ("scale", "clip", "unmatched"):
                if not float(getattr(tg, name)) >= 0:
                    raise ValueError(f"type_guidance.{name} must be >= 0, got {getattr(tg, name)}")
            if not sharp >= 0:
                raise ValueError(f"type_guidance.sharpness must be >= 0, got {sharp}")
            types = (float(tg.scale), float(tg.clip), sharp * float(self.pharm_feat_norm_constant), bool(tg.complementarity),
                     float(tg.unmatched))
        separation = None
        if min_separation is not None:
            d, w = float(min_separation), float(separation_weight)
            if not 0 <= d < math.inf:
                raise ValueError(f"min_separation must be finite and >= 0, got {min_separation}")
            if not 0 <= w < math.inf:
                raise ValueError(f"separation_weight must be finite and >= 0, got {separation_weight}")
            if not guided:
                raise ValueError("min_separation makes every batch guided: the caller's guided must say so")
            separation = (d, w)
        if (seeds is None) != (seed_level is None):
            raise ValueError("seeds and seed_level go together: a seeded run needs both")
        if seeds is None and seed_keep is not None:
            raise ValueError("seed_keep without seeds")
        if seeds is not None and pinned:
            raise ValueError("seeds together with pinned centers: use seed_keep")
        T = int(self.n_timesteps)
        return RunSpec(T=T, top=T if seeds is None else self._check_seed_level(seed_level), seeded=seeds is not None, fewstep=fewstep,
                       pin_resamples=int(pin_resamples), pin_jump=int(pin_jump), guide_scale=float(guide_scale),
                       guide_clip=float(guide_clip), guide_family=guide_family, guided=bool(guided), types=types, separation=separation)

    def _field_for_batch(self, g, pocket_field, radii=None):
        """PfEngine.field_next's arguments for a batched graph and a PocketField (None: None), checked before any device work.
        ``radii``: per graph of the batch a float or that graph's per-atom tensor (None: pocket_field.clash_radius for the whole
        batch).  Receptor features are the graphs' prot_ph_x (the pocket's frame) with the types prot_ph_h's argmax."""
        pf = pocket_field
        if pf is None:
            return None
        if not isinstance(pf, PocketField):
            raise ValueError(f"pocket_field must be a PocketField, got {type(pf).__name__}")
        from .analysis import complementarity_tables
        kw = dict(kappa=float(pf.kappa), type_sharpness=float(pf.type_sharpness) * float(self.pharm_feat_norm_constant),
                  w_clash=float(pf.clash_weight), w_comp=float(pf.comp_weight))
        counts = (g.prot_ptr[1:] - g.prot_ptr[:-1]).tolist()
        if radii is None and pf.clash_radius is not None:
            r = pf.clash_radius
            if torch.is_tensor(r):
                if r.numel() != int(g.prot_ptr[-1]):
                    raise ValueError(f"clash_radius has {r.numel()} entries for a batch of {int(g.prot_ptr[-1])} atoms")
                kw["atom_r"] = r.detach().float().reshape(-1).cpu()
            else:
                kw["atom_r"] = float(r)
        elif radii is not None:
            rows = []
            for i, (r, n) in enumerate(zip(radii, counts)):
                if torch.is_tensor(r):
                    if r.numel() != n:
                        raise ValueError(f"clash_radius has {r.numel()} entries for a pocket of {n} atoms (graph {i} of the batch)")
                    rows.append(r.detach().float().reshape(-1).cpu())
                else:
                    rows.append(torch.full((n,), float(r)))
            kw["atom_r"] = torch.cat(rows) if rows else torch.zeros(0)
        if float(pf.comp_weight) > 0:
            if g.prot_ph_x is None or g.prot_ph_h is None or g.prot_ph_ptr is None:
                raise ValueError("comp_weight > 0 needs receptor features on the graphs (prot_ph_x / prot_ph_h), and these have none: "
                                 "PDB input carries no receptor features; use comp_weight = 0 or a dataset graph")
            match, dist = complementarity_tables()
            if self.n_pharm_feats != match.shape[0]:
                raise ValueError(f"the complementarity tables are for {match.shape[0]} feature types; this model has {self.n_pharm_feats}")
            kw.update(ph=(g.prot_ph_ptr.cpu(), g.prot_ph_x.detach().float().cpu(), g.prot_ph_h.detach().argmax(dim=1).cpu()), match=match, dist=dist)
        return kw

    def _check_guide_family(self, guide_family):
        """``guide_family`` of sample / sample_given_receptor, checked before any device work: 'wide' (default) or 'tuned', which
        needs the tuned kernels' widths (n_hidden_scalars 128 / vector_size 16)."""
        if guide_family not in PfEngine.GUIDE_FAMILIES:
            raise ValueError(f"guide_family must be 'wide' or 'tuned', got {guide_family!r}")
        arch = self.dynamics._arch
        if guide_family == "tuned" and (arch.get("n_hidden_scalars", 128), arch.get("vector_size", 16)) != (128, 16):
            raise ValueError("guide_family='tuned' needs n_hidden_scalars 128 / vector_size 16; this model has "
                             f"{arch.get('n_hidden_scalars', 128)} / {arch.get('vector_size', 16)}: use guide_family='wide'")
        return guide_family

    def _fewstep(self, sample_steps, sampler, eta, spacing, pin_resamples=1, seed_level=None, pins=False, restraints=False):
        """The few-step keywords of sample / sample_given_receptor, checked before any device work: None without sample_steps,
        else (N, sampler, eta, spacing).  'ancestral' is eta = 1 (the default sampler), 'ddim' defaults to eta = 0, 'multistep'
        takes no eta and composes with seeds only."""
        if sample_steps is None:
            if sampler is not None or eta is not None or spacing is not None:
                raise ValueError("sampler, eta and spacing belong to a few-step run: pass sample_steps")
            return None
        sampler = "ancestral" if sampler is None else sampler
        spacing = "uniform" if spacing is None else spacing
        if sampler not in ("ancestral", "ddim", "multistep"):
            raise ValueError(f"sampler must be 'ancestral', 'ddim' or 'multistep', got {sampler!r}")
        if spacing not in ("uniform", "quadratic", "logsnr"):
            raise ValueError(f"spacing must be 'uniform', 'quadratic' or 'logsnr', got {spacing!r}")
        if pin_resamples > 1:
            raise ValueError("sample_steps together with pin_resamples > 1: resampling jumps over a strided plan are not supported")
        top = self.n_timesteps if seed_level is None else self._check_seed_level(seed_level)
        if not 1 <= int(sample_steps) <= top:
            raise ValueError(f"sample_steps must satisfy 1 <= sample_steps <= {top} (T, or the seed level of a seeded run), got {sample_steps}")
        if sampler == "multistep":
            if eta is not None:
                raise ValueError("sampler 'multistep' injects no noise and takes no eta")
            if pins or restraints:
                raise ValueError("sampler 'multistep' composes with seeds only: pinned centers (seed_keep included) and restraints "
                                 "need a first-order sampler ('ancestral' or 'ddim')")
            eta = 0.0
        elif sampler == "ancestral":
            if eta is not None and float(eta) != 1.0:
                raise ValueError("sampler 'ancestral' is eta = 1; use sampler='ddim' for another eta")
            eta = 1.0
        else:
            eta = 0.0 if eta is None else float(eta)
        if not 0.0 <= eta <= 1.0:
            raise ValueError(f"eta must lie in [0, 1], got {eta}")
        return int(sample_steps), sampler, float(eta), spacing

    def _fewstep_arrays(self, name, fewstep, top=None):
        """coef / pin / guide / ms: that per-step array of a few-step run, keyed by its plan (N, spacing, top) -- and by eta for the
        first-order coefficients, by the parameterisation for the multistep ones."""
        T = self.n_timesteps
        N, _, eta, spacing = fewstep
        top = T if top is None else int(top)
        gam = self.gamma.gamma
        levels = self._host_arrays(("levels", N, spacing, top), lambda: level_plan(T, N, spacing, top, gamma_table=gam))
        if name == "levels":
            return levels
        build = {"coef": lambda: PfEngine.coef_array(strided_coefficients(gam, T, levels, eta), range(N)),
                 "pin": lambda: PfEngine.pin_coef_array(pin_coefficients(gam, T, levels), range(N)),
                 "guide": lambda: PfEngine.guide_coef_array(guide_coefficients(gam, T, levels), range(N)),
                 "ms": lambda: PfEngine.ms_coef_array(multistep_coefficients(gam, T, levels, bool(self.endpoint_param_coord),
                                                                             bool(self.endpoint_param_feat)))}[name]
        extra = {"coef": (eta,), "ms": (bool(self.endpoint_param_coord), bool(self.endpoint_param_feat))}.get(name, ())
        return self._host_arrays((name, "fewstep", N, spacing, top) + extra, build)

    def _host_arrays(self, key, build):
        """The ctypes arrays of a run at this model's T (500-1000 structs an array; a plan's, a few thousand): built once per key."""
        key = (self.n_timesteps,) + tuple(key)
        if key not in self._arrays:
            self._arrays[key] = build()
        return self._arrays[key]

    def _step_arrays(self, name, top=None):
        """coef / pin / guide: that per-step coefficient array of a run that visits s = top-1 .. 0 (top None: T; a seeded run's
        top is its seed level)"""
        T = self.n_timesteps
        tabs, array = {"coef": (self.step_coefficients, PfEngine.coef_array),
                       "pin": (lambda: pin_coefficients(self.gamma.gamma, T), PfEngine.pin_coef_array),
                       "guide": (lambda: guide_coefficients(self.gamma.gamma, T), PfEngine.guide_coef_array)}[name]
        if top is None or int(top) == T:
            return self._host_arrays((name,), lambda: array(tabs(), reversed(range(T))))
        return self._host_arrays((name, int(top)), lambda: array(tabs(), reversed(range(int(top)))))

    def _plan_arrays(self, jump: int, resamples: int, top=None):
        """(n_ops, coef_arr, pin_coef_arr, op_arr, renoise_arr) of a resampled pinned run from level ``top`` down (None: this
        model's T; a seeded run's top is its seed level), per (jump, resamples, top)."""
        T = self.n_timesteps
        top = T if top is None else int(top)

        def build():
            plan = resample_plan(top, jump, resamples)
            pairs = [(op[1], op[2]) for op in plan if op[0] == "renoise"]
            return (len(plan),) + tuple(PfEngine.plan_arrays(plan, self.step_coefficients(), pin_coefficients(self.gamma.gamma, T),
                                                             renoise_coefficients(self.gamma.gamma, T, pairs)))
        return self._host_arrays(("plan", int(jump), int(resamples), top), build)

    def _check_seed_level(self, seed_level):
        if not 1 <= int(seed_level) <= self.n_timesteps:
            raise ValueError(f"seed_level must satisfy 1 <= seed_level <= {self.n_timesteps}, got {seed_level}")
        return int(seed_level)

    def _seed_fields(self, sizes, seeds, seed_keep, batch=False):
        """The pin fields that carry the seeds: per entry r a (flags [n], x [n,3], one-hot rows [n,nf]) from seeds[r] = (x [n,3],
        types [n]) and seed_keep[r] = the seed center indices that stay fixed (flag 3; seed_keep None: none).  An entry is a pocket
        of sample, or (``batch``, which only words the errors) a graph of sample_given_receptor's batch; sizes[r] lists the
        pharmacophore sizes requested of it, and each must be the seed's."""
        n = len(sizes)
        for name, v in (("seeds", seeds), ("seed_keep", seed_keep)):
            if v is not None and len(v) != n:
                raise ValueError(f"seeds (and seed_keep) need one entry per graph of the batch ({n})" if batch
                                 else f"{name} lists {len(v)} entries for {n} pockets")
        for r, sd in enumerate(seeds):
            if sd is None:
                raise ValueError(f"pocket {r} has no seed: a seeded run needs one seed per pocket")
        out = []
        for r, (x, types) in enumerate(seeds):
            x = torch.as_tensor(x, dtype=torch.float32).reshape(-1, 3)
            types = torch.as_tensor(types, dtype=torch.int64).reshape(-1)
            k = int(x.shape[0])
            other = [int(s) for s in sizes[r] if int(s) != k]
            if other:
                raise ValueError(f"pocket {r}: the seed has {k} centers but " + (
                    f"a pharmacophore of {other[0]} was requested (seeds of a different size than the sample are not supported)"
                    if batch else f"sizes {other} were requested"))
            if types.numel() != k:
                raise ValueError(f"pocket {r}: the seed has {k} positions and {types.numel()} types")
            if k and (int(types.min()) < 0 or int(types.max()) >= self.n_pharm_feats):
                raise ValueError(f"pocket {r}: seed types must be in 0..{self.n_pharm_feats - 1}")
            flags = torch.zeros(k, dtype=torch.int32)
            for i in (seed_keep[r] if seed_keep is not None else None) or []:
                if not 0 <= int(i) < k:
                    raise ValueError(f"pocket {r}: seed_keep names center {int(i)} of a seed of {k}")
                flags[int(i)] = 3
            out.append((flags, x, F.one_hot(types, self.n_pharm_feats).float()))
        return out

    def _with_seeds(self, ref_graphs, n_pharms, seeds, seed_keep):
        """sample(seeds=...): per pocket (x [n,3] in the pocket's frame, types [n] type indices).  The seed rides on the pin
        fields, which then hold values for ALL centers; seed_keep becomes the flags (3 for kept centers, 0 for the rest)."""
        return [self._with_pin_fields(g, *f) for g, f in zip(ref_graphs, self._seed_fields(n_pharms, seeds, seed_keep))]

    def _sample_enqueue(self, g, spec, init_pharm_com=None, visualize_trajectory=False, noise=None, lane: int = 0, restraints=None,
                        field=None, generator=None, type_restraints=None, pair_restraints=None):
        """First half of sample_given_receptor: upload the batch and enqueue the whole reverse process (asynchronous) on the
        current stream; ``lane`` > 0: on that lane's own handle (PharmRecDynamicsGVP.lane_engine).  What runs is ``spec``'s answer
        for this batch (RunSpec.batch): a pin flag set on the graph makes it pinned, a restraint in ``restraints`` (None or one
        list or None per graph of the batch), in ``type_restraints`` or ``pair_restraints``, ``field`` (_field_for_batch) or the
        spec's minimum separation guided.  A seeded run's graph holds the seed of EVERY
        center on pharm_pin_x / pharm_pin_h (the flags say which of them stay fixed).  ``noise`` None: the rows the run reads, one
        torch.randn on the model's device from ``generator``."""
        g = as_pocket_graph(g)
        dev = self.device
        guided = self._guided(restraints, field, type_restraints, pair_restraints, spec.separation)
        kind, n_ops, rows, arr, kw = spec.batch(self, self._has_pins(g), guided)
        if noise is not None and noise.shape[0] != rows:
            if spec.fewstep is not None:
                raise ValueError(f"a {spec.fewstep[1]} run of {n_ops} steps needs {rows} noise row(s), got {noise.shape[0]}")
            if kind == "resampled":
                raise ValueError(f"a resampled pinned run of {n_ops} ops (T = {spec.T}, jump {spec.pin_jump}, resamples "
                                 f"{spec.pin_resamples}) needs {rows} noise rows, got {noise.shape[0]}")
            if spec.seeded:
                raise ValueError(f"a seeded run of {n_ops} ops (seed level {spec.top}) needs {rows} noise rows, got {noise.shape[0]}")
            # (a full-length unseeded run has always ignored extra rows; the engine asserts that there are enough)
        if "pin_coef_arr" in kw and g.pharm_pin is not None:       # (a seeded multistep run carries its seed on these fields: no pins)
            kw["pins"] = (g.pharm_pin, g.pharm_pin_x, g.pharm_pin_h)
        if spec.seeded:
            kw["seed"] = (g.pharm_pin_x, g.pharm_pin_h, seed_coefficients(self.gamma.gamma, self.n_timesteps, spec.top))
        if guided:
            restraints = [None] * g.batch_size if restraints is None else restraints
            if len(restraints) != g.batch_size:
                raise ValueError(f"restraints lists {len(restraints)} entries for a batch of {g.batch_size} graphs")
            kw["restraints"] = restraints
            if field is not None:
                kw["field"] = field
            if type_restraints is not None and len(type_restraints) != g.batch_size:
                raise ValueError(f"type_restraints lists {len(type_restraints)} entries for a batch of {g.batch_size} graphs")
            types = spec.types_kwargs(type_restraints)      # (every guided batch of a call with type guidance carries it)
            if types is not None:
                kw["types"] = types
            if pair_restraints is not None and len(pair_restraints) != g.batch_size:
                raise ValueError(f"pair_restraints lists {len(pair_restraints)} entries for a batch of {g.batch_size} graphs")
            pairs = spec.pairs_arg(pair_restraints, g.batch_size)
            if pairs is not None:
                kw["pairs"] = pairs
        if noise is None:
            noise = torch.randn(rows, g.num_nodes("pharm"), 3 + self.n_pharm_feats, device=dev, generator=generator)
        if lane == 0:
            eng = self.dynamics.bind_graph(g)
        else:
            eng = self.dynamics.lane_engine(lane)
            eng.set_batch(g.prot_x, g.prot_h, g.prot_ptr, g.pharm_ptr, g.pp_src, g.pp_dst, pocket_uid=g.pocket_uid)
        com = None
        if init_pharm_com is not None:
            com = init_pharm_com if init_pharm_com.is_cuda else init_pharm_com.float().pin_memory().to(dev, non_blocking=True)
        res = eng.sample(arr, n_ops, noise if noise.is_cuda else noise.float().pin_memory().to(dev, non_blocking=True),
                         init_pharm_com=com, ep_coord=self.endpoint_param_coord,
                         ep_feat=self.endpoint_param_feat, feat_norm_constant=float(self.pharm_feat_norm_constant),
                         trajectory=visualize_trajectory, **kw)
        # results go to pinned host memory with copies enqueued right behind the batch's kernels, and an event marks their
        # completion: whatever is enqueued afterwards (the next batch) does not delay the fetch of this one
        host = tuple(None if r is None else torch.empty(r.shape, dtype=r.dtype, pin_memory=True).copy_(r, non_blocking=True)
                     for r in res)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(dev))
        return g, host, visualize_trajectory, done, eng, kw.get("pairs")

    def _sample_fetch(self, pending):
        """Results of an enqueued batch on the host (waits for that batch only).  The run's validity word arrived with them
        (pf_sample_end): an exchange time-out inside a merged launch raises PfError HERE, before anything is built from x_0 / h_0."""
        g, host, traj, done, eng, pairs = pending
        done.synchronize()
        eng.sample_status()
        return g, host, traj, pairs

    def _sample_finish(self, pending) -> List[SampledPharmacophore]:
        """Second half: per-graph SampledPharmacophores (host work only once the results are fetched)."""
        g, res, visualize_trajectory = pending[:3]
        pairs = pending[3] if len(pending) > 3 else None        # the batch's pair restraints per graph: their final energy goes along
        x0, h0 = res[0].cpu(), res[1].cpu()
        traj_x = res[2].cpu() if visualize_trajectory else None
        traj_h = res[3].cpu() if visualize_trajectory else None
        out: List[SampledPharmacophore] = []
        g_cpu = g.to("cpu")
        for gi, g_i in enumerate(unbatch(g_cpu)):
            f0, f1 = int(g.pharm_ptr[gi]), int(g.pharm_ptr[gi + 1])
            g_i.pharm_x0, g_i.pharm_h0 = x0[f0:f1], h0[f0:f1]
            kwargs = {"g": g_i, "pharm_type_map": self.ph_type_map}
            if visualize_trajectory:
                kwargs["traj_frames"] = (traj_x[:, f0:f1], traj_h[:, f0:f1])
            out.append(SampledPharmacophore(**kwargs))
            if pairs is not None:
                out[-1].pair_energy, out[-1].pair_violations = pair_restraint_energy(x0[f0:f1], pairs[gi])
        return out

    def _with_pins(self, ref_graphs, n_pharms, pinned):
        """sample(pinned=...): per pocket None or (x [k,3] in the pocket's frame, types [k] type indices, flags [k] or None =
        pin both).  The k given centers become the FIRST k centers of every copy of that pocket (copy_graph pads the rest
        with free centers); a requested size below k is refused here, before any device work."""
        if len(pinned) != len(ref_graphs):
            raise ValueError(f"pinned lists {len(pinned)} entries for {len(ref_graphs)} pockets")
        out = []
        for r, (g, pin) in enumerate(zip(ref_graphs, pinned)):
            if pin is None:
                out.append(g)
                continue
            x, types, flags = pin
            x = torch.as_tensor(x, dtype=torch.float32).reshape(-1, 3)
            types = torch.as_tensor(types, dtype=torch.int64).reshape(-1)
            k = int(x.shape[0])
            flags = torch.full((k,), 3, dtype=torch.int32) if flags is None else torch.as_tensor(flags, dtype=torch.int32).reshape(-1)
            if types.numel() != k or flags.numel() != k:
                raise ValueError(f"pocket {r}: {k} pinned positions, {types.numel()} types, {flags.numel()} flags")
            if k and (int(types.min()) < 0 or int(types.max()) >= self.n_pharm_feats or int(flags.min()) < 0 or int(flags.max()) > 3):
                raise ValueError(f"pocket {r}: pinned types must be in 0..{self.n_pharm_feats - 1} and flags in 0..3")
            small = [int(n) for n in n_pharms[r] if int(n) < k]
            if small:
                raise ValueError(f"pocket {r}: {k} centers are pinned but sizes {small} were requested")
            out.append(self._with_pin_fields(g, flags, x, F.one_hot(types, self.n_pharm_feats).float()))
        return out

    def sample(self, ref_graphs: List[PocketGraph], n_pharms: List[List[int]], max_batch_size: int = 32,
               init_pharm_com: torch.Tensor = None, visualize_trajectory: bool = False,
               rank: int = 0, world_size: int = 1, noise=None, lanes: int = None,
               pinned=None, pin_resamples: int = 1, pin_jump: int = 10, restraints=None, guide_scale: float = 1.0,
               guide_clip: float = 0.0, seeds=None, seed_level: int = None, seed_keep=None,
               score_levels: int = None, sample_steps: int = None, sampler: str = None, eta: float = None,
               spacing: str = None, guide_family: str = "wide", pocket_field=None, type_restraints=None,
               type_guidance=None, pair_restraints=None, min_separation: float = None,
               separation_weight: float = 1.0, consensus=None) -> List[List[SampledPharmacophore]]:
        """pharmacodiff.py:516-578: one pocket copy per requested pharmacophore, flattened in pocket order and cut into
        batches of ``max_batch_size`` in list order.

        With ``world_size`` > 1 whole BATCHES are dealt over the ranks (greedy by protein-protein edge count,
        sharding.shard_by_work; no data-path collective): a batch holds the same graphs, in the same order, whatever the
        number of GPUs, so every sample is bitwise the one a single GPU produces.  Each rank returns only its own
        samples, still grouped per pocket (shorter or empty lists for the others).

        ``noise``: None -- batch i draws its [T+1, Nf_i, 3+nf] Gaussians from a device generator seeded with
        (one draw from torch's global CPU generator) + i, i.e. reproducible under torch.manual_seed and independent of
        rank / world_size when the ranks share the seed; or a list with one such tensor per batch (replaying a
        reference run: tests/golden/sample_multi.npz).

        ``pinned``: None, or one entry per pocket -- None or (x [k,3], types [k], flags [k] or None): every pharmacophore
        of that pocket is completed around these k centers, which are its first k (flag bit 0: position given, bit 1: type
        given; None = both).  Raises ValueError when a requested size is below k.

        ``pin_resamples`` r, ``pin_jump`` j: with r > 1 every batch holding a pinned graph runs with resampling jumps
        (schedule.resample_plan(T, j, r): n_ops ~ r T ops instead of T, i.e. about r times the work of a pinned run), so that the
        free centers can react to the given ones; its noise has n_ops + 1 rows.  Batches of free graphs run the default path with
        T + 1 rows, as without them.

        ``restraints``: None, or one entry per pocket -- None or a list of (kind, center, point, radius, weight) with kind
        'attract' / 'repel', center a center index of the pharmacophore or None for every center, point in the pocket's frame
        (pocket_io.parse_restraints reads them from text).  Copies of a pocket share its restraints.  A batch with a restraint
        runs guided (pf_sample_guided: restraint energies on the predicted clean centers shift every step's posterior mean by
        ``guide_scale`` times the posterior variance times the energy's gradient through the network, each center's shift
        clipped to ``guide_clip`` angstroms when that is positive); its steps run the width-generic training forward and its
        input gradients and cost several times a default step.  Batches without one run the default path.
        ``guide_family``: 'wide' (the default) or 'tuned' -- a model of the tuned widths (128 / 16) then runs the guided steps'
        training forward and input gradients on the tuned kernels; any other model is a ValueError.
        Composes with ``pinned``; together with ``pin_resamples`` > 1 it is a ValueError.

        ``pocket_field``: None or a PocketField -- clash avoidance against the pocket's own atoms and / or complementarity to its
        receptor features, added to the restraints' energy.  EVERY batch then runs guided, with or without
        restraints; it composes with ``pinned``, ``restraints``, ``seeds`` and ``sample_steps`` with 'ancestral' / 'ddim', and is
        refused like restraints with sampler 'multistep' and with ``pin_resamples`` > 1.  ``comp_weight`` > 0 on graphs without
        prot_ph_x / prot_ph_h is a ValueError.  On its own it steers coordinates only.

        ``type_restraints``: None, or one entry per pocket -- None or a list of (type, center, point, radius, weight): type a name
        of the model's ph_type_map or an index, center a center index or None for every center, point in the pocket's frame,
        radius 0 for no spatial condition (pocket_io.parse_type_restraints reads them from text).  Inside the sphere a center
        takes that type or is pushed out; together with an 'attract' restraint on the same sphere: "a center of this
        type within radius of point".  Copies of a pocket share its type restraints; a batch with one runs guided.
        ``type_guidance``: None or a TypeGuidance -- scale, clip and sharpness of the feature guidance, and ``complementarity``:
        the pocket field's complementarity energy steers the types too (without a ``pocket_field`` with comp_weight > 0 a
        ValueError).  Every guided batch of a call with type guidance carries it.  Composes with ``pinned`` (a type-pinned center
        keeps its type), ``restraints``, ``pocket_field``, ``seeds``, first-order ``sample_steps`` and both ``guide_family``
        values; refused like restraints with sampler 'multistep' and with ``pin_resamples`` > 1.

        ``pair_restraints``: None, or one entry per pocket -- None or a list of (i, j, lo, hi, weight): i, j center indices of the
        pharmacophore, or None / '*' / a negative index for every center; the distance of every covered pair of centers of one
        sample is held in lo .. hi (hi = inf: no upper bound) by weight * (max(0, lo - rho)^2 + max(0, rho - hi)^2) on the
        predicted clean centers (pocket_io.parse_pair_restraints reads them from text).  A position-pinned center
        stands at its given position and is not moved.  Copies of a pocket share its pair restraints; a batch with one runs guided.
        ``min_separation`` d with ``separation_weight`` w (default 1): "no two centers closer than d" -- (*, *, d, inf, w) on
        every graph, behind its pair restraints.  EVERY batch then runs guided, like a pocket field.  Both compose with
        ``pinned``, ``restraints``, ``pocket_field``, ``type_restraints``, ``seeds``, first-order ``sample_steps`` and both
        ``guide_family`` values; refused like restraints with sampler 'multistep' and with ``pin_resamples`` > 1.  An index that a
        requested size does not have is a ValueError.  Every returned SampledPharmacophore of a batch that carried pair restraints
        has ``pair_energy`` / ``pair_violations``: analysis.pair_restraint_energy of its final centers.

        ``seeds`` with ``seed_level`` a, 1 <= a <= T: variations of given pharmacophores (partial diffusion, pf_sample_seed_next)
        -- one (x [n,3], types [n]) per pocket, every pocket must have one and every requested size of it must equal n.  Each
        seed is noised forward to level a and only the steps a-1 .. 0 are run: a small a gives close analogues, a large a loose
        ones, and the run costs a / T of a default run.  Its noise has a + 1 rows.  Copies of a pocket share its seed.
        ``seed_keep``: None, or per pocket a list of seed center indices that stay fixed in position and type -- the run is then
        a pinned run with these centers flagged, and they come back bit for bit.  With ``pin_resamples`` > 1 such a run follows
        schedule.resample_plan(a, j, r); with ``restraints`` it is guided.  Together with ``pinned`` it is a ValueError.

        ``sample_steps`` N: a few-step run -- the reverse process visits only the N + 1 levels of schedule.level_plan(T, N,
        ``spacing``) ('uniform', 'quadratic' or 'logsnr'; from the seed level down in a seeded run, which needs N <= a) and costs
        N network evaluations.  ``sampler``: 'ancestral' (the default; the reference's posterior between the plan's levels, eta = 1),
        'ddim' (``eta`` in [0, 1], default 0: no injected noise) -- both run the default path's steps with strided coefficients
        (schedule.strided_coefficients) and compose with ``pinned``, ``restraints`` and ``seeds``; their noise has N + 1 rows -- or
        'multistep' (a second-order multistep solver of the probability-flow ODE, schedule.multistep_coefficients and
        pf_sample_ms: 1 noise row, the initial draw), which composes with ``seeds`` only: with pins (``seed_keep`` included) or
        restraints it is a ValueError.  Together with ``pin_resamples`` > 1 every few-step run is a ValueError.  Trajectories have
        N + 1 frames.  How good an N-step sample is depends on the trained weights and is not measured by this project.

        ``lanes`` (default ``self.sample_lanes``; None = 2, or 4 when the batches hold at most 32 graphs): batches in flight at
        once, each on its own HIP stream and handle.  Four of
        the five launches of a batched step occupy part of the chip, so independent batches overlap (2 lanes: +16 % at
        batches of 128, +34 % at batches of 32; 4 lanes: +27 % / +58 %); a batch's result does not depend on the lane it ran on.

        ``score_levels`` K: every returned SampledPharmacophore carries ``.score``, the PharmacophoreScore of its final frame at K
        stratified levels (score(), uniform weighting, seed 0) -- a second pass behind the sampling, which it leaves bit for bit
        as it is without.  None (the default): no scoring, ``.score`` stays None.

        ``consensus``: True, or a dict of consensus()'s keywords -- the call returns (samples, sets), sets being consensus() of the
        samples this rank returns, one SampleSet per pocket (None for a pocket of which it holds none); the sampling is bit for
        bit what it is without.  None / False (the default): the samples alone, as before."""
        type_restraints = self._type_restraints(type_restraints, len(ref_graphs), "pockets")
        pair_restraints = self._pair_restraints(pair_restraints, len(ref_graphs), "pockets", n_pharms, int(min_separation is not None))
        spec = self._run_spec(pins=pinned is not None and any(p is not None for p in pinned),
                              guided=self._guided(restraints, pocket_field, type_restraints, pair_restraints, min_separation),
                              pinned=pinned is not None,
                              pin_resamples=pin_resamples,
                              pin_jump=pin_jump, guide_scale=guide_scale, guide_clip=guide_clip, seeds=seeds, seed_level=seed_level,
                              seed_keep=seed_keep, score_levels=score_levels, sample_steps=sample_steps, sampler=sampler, eta=eta,
                              spacing=spacing, guide_family=guide_family, pocket_field=pocket_field, type_guidance=type_guidance,
                              typed=type_restraints is not None, min_separation=min_separation, separation_weight=separation_weight)
        for r, rs in enumerate(type_restraints or []):
            for _, c, _, _, _ in (rs or []):
                if c is not None:
                    small = [int(n) for n in n_pharms[r] if int(n) <= c]
                    if small:
                        raise ValueError(f"pocket {r}: a type restraint names center {c} but sizes {small} were requested")
        scored_graphs = ref_graphs
        from .sharding import shard_by_work
        ref_graphs = [as_pocket_graph(g) for g in ref_graphs]
        n_receptors = len(ref_graphs)
        if n_receptors == 0:
            return ([], []) if consensus else []
        if restraints is not None:
            if len(restraints) != n_receptors:
                raise ValueError(f"restraints lists {len(restraints)} entries for {n_receptors} pockets")
            restraints = [list(r) if r else None for r in restraints]
            if not any(restraints):
                restraints = None
            for r, rs in enumerate(restraints or []):
                for _, c, _, _, _ in (rs or []):
                    if c is not None and c != "*" and int(c) >= 0:
                        small = [int(n) for n in n_pharms[r] if int(n) <= int(c)]
                        if small:
                            raise ValueError(f"pocket {r}: a restraint names center {int(c)} but sizes {small} were requested")
        radii = None
        if pocket_field is not None:
            if not isinstance(pocket_field, PocketField):
                raise ValueError(f"pocket_field must be a PocketField, got {type(pocket_field).__name__}")
            r = pocket_field.clash_radius
            if r is not None:
                radii = list(r) if isinstance(r, (list, tuple)) else [r] * n_receptors
                if len(radii) != n_receptors:
                    raise ValueError(f"clash_radius lists {len(radii)} entries for {n_receptors} pockets")
                for i, (ri, gi) in enumerate(zip(radii, ref_graphs)):
                    if torch.is_tensor(ri) and ri.numel() != gi.num_nodes("prot"):
                        raise ValueError(f"pocket {i}: clash_radius has {ri.numel()} entries for {gi.num_nodes('prot')} atoms")
            if float(pocket_field.comp_weight) > 0:
                for i, gi in enumerate(ref_graphs):
                    if gi.prot_ph_x is None or gi.prot_ph_h is None:
                        raise ValueError(f"pocket {i} has no receptor features (prot_ph_x / prot_ph_h): comp_weight > 0 needs them "
                                         "(PDB input carries none; use comp_weight = 0 or a dataset graph)")
        if pinned is not None:
            ref_graphs = self._with_pins(ref_graphs, n_pharms, pinned)
        if seeds is not None:
            ref_graphs = self._with_seeds(ref_graphs, n_pharms, seeds, seed_keep)
        if init_pharm_com is None:
            init_pharm_com = torch.stack([g.prot_x.mean(dim=0) for g in ref_graphs], dim=0)
        # the requested graphs in pocket order: (pocket, number of centers); the copies themselves are made batch by batch
        # inside the pipeline (30,000 graph objects up front cost a dataset-scale run most of a second before the device starts)
        graph_ref_idx = [rec_idx for rec_idx in range(n_receptors) for _ in n_pharms[rec_idx]]
        graph_size = [int(n) for rec_idx in range(n_receptors) for n in n_pharms[rec_idx]]
        n_graphs = len(graph_ref_idx)

        def make_batch(idx):
            gs, a = [], 0
            while a < len(idx):                         # runs of one pocket: one copy_graph call each (its copies share a pocket_uid)
                b = a
                while b < len(idx) and graph_ref_idx[idx[b]] == graph_ref_idx[idx[a]]:
                    b += 1
                gs.extend(copy_graph(ref_graphs[graph_ref_idx[idx[a]]], n_copies=b - a,
                                     pharm_feats_per_copy=torch.tensor([graph_size[i] for i in idx[a:b]])))
                a = b
            return batch_graphs(gs)
        batches = [list(range(s0, min(s0 + max_batch_size, n_graphs))) for s0 in range(0, n_graphs, max_batch_size)]
        if world_size > 1:
            epp = [int(g.pp_src.numel()) for g in ref_graphs]
            work = [sum(epp[graph_ref_idx[i]] + 1 for i in idx) for idx in batches]
            mine = shard_by_work(work, world_size)[rank]
        else:
            mine = list(range(len(batches)))
        base_seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if noise is None else 0
        # every graph's initial center of mass on the device with ONE copy before the pipeline starts (a batch is a
        # contiguous range of graphs); per-batch host -> device copies would each wait for the batch in flight
        coms_dev = init_pharm_com[graph_ref_idx].to(self.device, torch.float32) if n_graphs else None
        sampled = {}
        # Pipeline over the batches: the host work of a batch (collating the next one, splitting the previous one's results
        # into SampledPharmacophores) runs while the device works on another batch.  Nothing in it waits for the device
        # except the fetch of a finished batch: uploads go through pinned memory, pf_set_pocket_batch is asynchronous, and
        # the one workspace of the handle is reused in stream order.  The batched graph stays on the host: the engine
        # uploads what it needs once, and the per-graph views are host tensors anyway.
        def finish(done):
            for i, p in zip(done[0], self._sample_finish(done[1])):
                sampled[i] = p
        want = self.sample_lanes if lanes is None else lanes
        if want is None:                                # batches of up to 32 graphs leave more of the chip idle: four lanes (811 k against
            want = 4 if max((len(batches[bi]) for bi in mine), default=0) <= 32 else 2      # 737 k sample-steps/s with two); larger ones: two
        n_lanes = max(1, min(int(want), len(mine)))
        cur = torch.cuda.current_stream(self.device)
        streams = [cur] + [torch.cuda.Stream(device=self.device) for _ in range(n_lanes - 1)]
        for st in streams[1:]:
            st.wait_stream(cur)                         # coms_dev (and the caller's earlier work) are ready
        pending = []                                    # enqueued batches, oldest first: at most n_lanes
        for k, bi in enumerate(mine):
            idx = batches[bi]
            batch_g = make_batch(idx)
            init_coms = coms_dev[idx[0]:idx[-1] + 1]
            lane = k % n_lanes
            with torch.cuda.stream(streams[lane]):
                # the noise rows this batch's run reads (RunSpec.batch) are drawn from its own generator, or given
                gen = torch.Generator(device=self.device).manual_seed(base_seed + bi) if noise is None else None
                # the bind is asynchronous (stream-ordered behind the lane's previous batch), nothing here waits for the device
                batch_r = [restraints[graph_ref_idx[i]] for i in idx] if restraints is not None else None
                field = self._field_for_batch(batch_g, pocket_field, None if radii is None else [radii[graph_ref_idx[i]] for i in idx])
                batch_t = [type_restraints[graph_ref_idx[i]] for i in idx] if type_restraints is not None else None
                batch_p = [pair_restraints[graph_ref_idx[i]] for i in idx] if pair_restraints is not None else None
                enq = self._sample_enqueue(batch_g, spec, init_coms, visualize_trajectory, None if noise is None else noise[bi],
                                           lane=lane, restraints=batch_r, field=field, generator=gen, type_restraints=batch_t,
                                           pair_restraints=batch_p)
            pending.append((idx, enq))
            if len(pending) > n_lanes:                  # every lane has a batch queued behind the one it runs: fetch the oldest
                i0, e0 = pending.pop(0)                 # (its lane goes straight into the batch just enqueued) and split it on
                finish((i0, self._sample_fetch(e0)))    # the host while the device works
        for i0, e0 in pending:
            finish((i0, self._sample_fetch(e0)))
        for st in streams[1:]:
            cur.wait_stream(st)
        per_pocket, end = [], 0
        for rec_idx in range(n_receptors):
            start, end = end, end + len(n_pharms[rec_idx])
            per_pocket.append([sampled[i] for i in range(start, end) if i in sampled])
        if score_levels is not None:
            cands = [[(p.ph_coords, p.ph_feats_idxs) for p in ps] for ps in per_pocket]
            scores = self.score(scored_graphs, cands, levels=_score_levels(self.n_timesteps, int(score_levels)), max_batch_size=max_batch_size)
            for ps, sc in zip(per_pocket, scores):
                for p, v in zip(ps, sc):
                    p.score = v
        if consensus:
            return per_pocket, self.consensus(per_pocket, **(consensus if isinstance(consensus, dict) else {}))
        return per_pocket

    # -- what the samples of a pocket agree on (pf_sample_set_analyze) ------------------------------
    def consensus(self, per_pocket_samples, sigma: float = 1.0, tolerance: float = 1.5, threshold: float = 0.5,
                  min_support: float = 0.5, device=None) -> List[Optional[SampleSet]]:
        """One SampleSet per pocket from what sample() returns (per pocket a list of SampledPharmacophore) or from per-pocket lists
        of (x [n, 3], type indices [n]) pairs: the typed Gaussian-overlap Tanimoto (``sigma``) between the samples of a pocket,
        the support of every center (the number of other samples with a center of its type within ``tolerance``), Taylor-Butina
        clusters at ``threshold`` and the consensus pharmacophore of each cluster, whose centers print when their support is at
        least ``min_support``.  Samples of one pocket share its frame and nothing is aligned: sets of different
        pockets do not compare.  A set has at most 1024 samples of at most 64 centers (ValueError).  Runs on the device when the
        model is on one (many pockets per call, chunked under the call's cap), else on the host through analysis.py;
        ``device``: 'cpu' forces the host path.  A pocket without samples gives None."""
        dev = torch.device(device) if device is not None else self.device
        eng = self.dynamics.engine() if torch.device(dev).type == "cuda" else None
        return sample_sets(per_pocket_samples, eng, sigma, tolerance, threshold, min_support)

    # -- screening a pharmacophore library (pf_pharm_align) -------------------------------------------
    def screen(self, queries, library, top_k: int = 10, min_match: float = 0.0, sigma: float = 1.0, tolerance: float = 1.5,
               refine: int = 4, device=None) -> List[List[ScreenHit]]:
        """One list of ScreenHit per query, best first: ``library`` (a PharmacophoreLibrary) is superposed rigidly onto every
        query -- samples, ConsensusPharmacophore objects or (x, types) pairs of at most 16 centers (ValueError above that cap) --
        and ranked by the typed Gaussian-overlap Tanimoto of the sample sets (``sigma``) after the superposition.
        Only entries with n_matched >= ceil(min_match * n_q) qualify (n_matched: query centers with a same-type entry center
        within ``tolerance``); the order is by sim, then entry index; ``refine``: refinement rounds.  Proper rotations only and
        exact types; the result is the best of a discrete seed set plus a local refinement.  Runs on the device when the model
        is on one (chunked under the call's pair cap), else on the host through analysis.py; ``device``: 'cpu' forces the host."""
        dev = torch.device(device) if device is not None else self.device
        eng = self.dynamics.engine() if torch.device(dev).type == "cuda" else None
        return screen_library(queries, library, eng, top_k, min_match, sigma, tolerance, refine)

    # -- scoring given pharmacophores (pf_score) ---------------------------------------------------
    def score(self, ref_graphs: List[PocketGraph], pharmacophores, levels=None, weighting: str = 'uniform', noise=None, seed: int = 0,
              max_batch_size: int = 32) -> List[List[PharmacophoreScore]]:
        """How plausible the model finds GIVEN pharmacophores for their pockets.  ``pharmacophores[i]``: a list of (x [n,3] in the
        frame of pocket i, types [n] type indices).  Every candidate is noised to each of ``levels`` (default: every level
        1 .. T; schedule.score_levels(T, K) for a stratified subset) and the network's prediction error there is a term of its
        variational bound; the terms are weighted (``weighting``: 'uniform' -- the per-graph training loss, every
        parameterisation -- or 'vlb', schedule.score_weights) and summed.  Batches are built as sample() builds them: one copy
        of the pocket per candidate, in pocket order, cut into batches of ``max_batch_size``; copies of a pocket share conv
        layer 0's protein->protein messages.  ``noise``: None -- batch i draws [L, Nf_i, 3 + nf] Gaussians from a
        torch.Generator(seed + i) on the host, so a candidate's score depends on the batch it is in only through its noise: the same
        candidates in the same order with the same ``max_batch_size`` and seed give the same scores --;
        or a list with one such tensor per batch.  Returns, per pocket, a list of PharmacophoreScore (LOWER per_center is
        better; totals compare candidates of one size, there is no size prior in them).  A candidate of more than 64 centers,
        or of none, is a ValueError naming it."""
        # (pins a graph may carry are the sampler's: a scoring bind takes none)
        ref_graphs = [dataclasses.replace(as_pocket_graph(g), pharm_pin=None, pharm_pin_x=None, pharm_pin_h=None) for g in ref_graphs]
        if len(pharmacophores) != len(ref_graphs):
            raise ValueError(f"pharmacophores lists {len(pharmacophores)} entries for {len(ref_graphs)} pockets")
        T, nf = self.n_timesteps, self.n_pharm_feats
        lv = _score_levels(T) if levels is None else [int(t) for t in levels]
        if not lv or min(lv) < 0 or max(lv) > T:
            raise ValueError(f"levels must be a non-empty list of integers in 0..{T}")
        w_pos, w_feat = _score_weights(self.gamma.gamma, T, lv, weighting, bool(self.endpoint_param_coord), bool(self.endpoint_param_feat))
        flat = []                                       # (pocket, x, one-hot rows)
        for r, cands in enumerate(pharmacophores):
            for j, (x, types) in enumerate(cands):
                x = torch.as_tensor(x, dtype=torch.float32).reshape(-1, 3)
                types = torch.as_tensor(types, dtype=torch.int64).reshape(-1)
                n = int(x.shape[0])
                if n < 1 or n > 64:
                    raise ValueError(f"pocket {r}, pharmacophore {j}: {n} centers (a candidate has 1 to 64)")
                if types.numel() != n or int(types.min()) < 0 or int(types.max()) >= nf:
                    raise ValueError(f"pocket {r}, pharmacophore {j}: {n} positions need {n} types in 0..{nf - 1}")
                flat.append((r, x.cpu(), F.one_hot(types.cpu(), nf).float()))
        out = [[] for _ in ref_graphs]
        tabs = self._loss_tables()
        for bi, s0 in enumerate(range(0, len(flat), max_batch_size)):
            chunk = flat[s0:s0 + max_batch_size]
            gs, a = [], 0
            while a < len(chunk):                       # runs of one pocket: one copy_graph call each (its copies share a pocket_uid)
                b = a
                while b < len(chunk) and chunk[b][0] == chunk[a][0]:
                    b += 1
                gs.extend(copy_graph(ref_graphs[chunk[a][0]], n_copies=b - a,
                                     pharm_feats_per_copy=torch.tensor([c[1].shape[0] for c in chunk[a:b]])))
                a = b
            g = batch_graphs(gs)
            x0, h0 = torch.cat([c[1] for c in chunk]), torch.cat([c[2] for c in chunk])
            Nf = int(x0.shape[0])
            if noise is None:
                nz = torch.randn(len(lv), Nf, 3 + nf, generator=torch.Generator().manual_seed(int(seed) + bi))
            else:
                nz = noise[bi]
                if tuple(nz.shape) != (len(lv), Nf, 3 + nf):
                    raise ValueError(f"batch {bi}: noise of shape {(len(lv), Nf, 3 + nf)} expected, got {tuple(nz.shape)}")
            self.dynamics._batch_key = None             # always a fresh bind: a sampling run may hold the handle on this very batch
            eng = self.dynamics.bind_graph(g)
            sc, tm = eng.score(x0, h0, lv, nz, w_pos, w_feat, tabs[0], tabs[1], T, feat_norm=float(self.pharm_feat_norm_constant),
                               remove_com=bool(self.remove_com), ep_coord=bool(self.endpoint_param_coord),
                               ep_feat=bool(self.endpoint_param_feat), terms=True)
            sc, tm = sc.cpu(), tm.cpu()
            for k, c in enumerate(chunk):
                out[c[0]].append(PharmacophoreScore(c[1].shape[0], lv, sc[k, 0], sc[k, 1], tm[:, k, :].clone()))
        return out

    # -- training-loss forward (pharmacodiff.py:162-243), evaluation only ---------------------------
    def _check_injected_t(self, t_int, B):
        """A caller-supplied t_int indexes tables of n_timesteps + 1 entries on the device: refuse anything else here (the
        values the module draws itself, randint(0, T), need no check and no synchronisation)."""
        if t_int.numel() != B:
            raise ValueError(f"t_int has {t_int.numel()} entries for a batch of {B} graphs")
        lo, hi = int(t_int.min()), int(t_int.max())
        if lo < 0 or hi > self.n_timesteps:
            raise ValueError(f"t_int must lie in [0, {self.n_timesteps}], got [{lo}, {hi}]")

    def forward(self, g, phase: str = 'train', t_int: torch.Tensor = None, eps: Dict[str, torch.Tensor] = None):
        """Losses and metrics of one batch (pharmacodiff.py:162-243) with the dynamics -- and, when autograd is on,
        its backward -- evaluated by the HIP kernels.  ``t_int`` / ``eps`` inject the random draws."""
        g = as_pocket_graph(g)
        dev = self.device
        self.__dict__["_fused_sums"] = None
        if self.fused_loss and dev.type == "cuda":
            return self._forward_fused(g, phase, t_int, eps)
        bidx = get_batch_idxs(g)
        bp, br = bidx['pharm'].to(dev), bidx['prot'].to(dev)
        B = g.batch_size
        # the (host) ptr array on the device, cached on the graph object like the batch indices: a pageable host -> device
        # copy waits for everything enqueued before it, i.e. for the previous training step
        ck = g.__dict__.get("_ptrf_cache")
        if ck is None or ck[0] != (str(dev), g.pharm_ptr.data_ptr(), int(g.pharm_ptr[-1])):
            ck = ((str(dev), g.pharm_ptr.data_ptr(), int(g.pharm_ptr[-1])), g.pharm_ptr.to(dev))
            g.__dict__["_ptrf_cache"] = ck
        ptr_f = ck[1]

        def seg_mean(x):
            out = torch.zeros(B, 3, device=dev).index_add_(0, bp, x)
            return out / (ptr_f[1:] - ptr_f[:-1]).clamp(min=1).unsqueeze(1)

        h0 = g.pharm_h0.to(dev) / self.pharm_feat_norm_constant
        com = seg_mean(g.pharm_x0.to(dev))
        x0 = g.pharm_x0.to(dev) - com[bp]
        prot_x = g.prot_x.to(dev) - com[br]
        if t_int is None:
            t_int = torch.randint(0, self.n_timesteps, size=(B,), device=dev)
        else:
            self._check_injected_t(t_int, B)
        t = t_int.to(dev).float() / self.n_timesteps
        if eps is None:
            eps = {'h': torch.randn(h0.shape, device=dev), 'x': torch.randn(x0.shape, device=dev)}
        eps = {k: v.to(dev) for k, v in eps.items()}
        gamma_t = self.gamma(t)
        alpha_t = self.alpha(gamma_t)[bp][:, None]
        sigma_t = self.sigma(gamma_t)[bp][:, None]
        x_t = alpha_t * x0 + sigma_t * eps['x']
        h_t = alpha_t * h0 + sigma_t * eps['h']
        if self.remove_com:
            c = seg_mean(x_t)
            x_t = x_t - c[bp]
            prot_x = prot_x - c[br]
            sampled_com = c[bp]
        h_dyn, x_dyn = self.dynamics.run(g, x_t, h_t, t, prot_x)
        if self.endpoint_param_feat:
            h_0_pred = h_dyn
            h_loss = F.cross_entropy(h_0_pred, h0.argmax(dim=1), reduction='none')
        else:
            h_loss = (eps['h'] - h_dyn).square().sum(dim=1)
            h_0_pred = (h_t - sigma_t * h_dyn) / alpha_t
        if self.endpoint_param_coord:
            if self.remove_com:
                x_dyn = x_dyn + sampled_com
            x_0_pred = x_dyn
            x_loss = (x_0_pred - x0).square().sum(dim=1)
        else:
            x_loss = (eps['x'] - x_dyn).square().sum(dim=1)
            x_0_pred = (x_t - sigma_t * x_dyn) / alpha_t
        weight_metric = 1 - t[bp]
        weight_loss = weight_metric if self.weighted_loss else torch.ones_like(weight_metric)
        losses = {phase + ' pos loss': (x_loss * weight_loss).sum() / eps['x'].numel(),
                  phase + ' feat loss': (h_loss * weight_loss).sum() / eps['h'].numel()}
        with torch.no_grad():
            err = (x_0_pred - x0).square().sum(dim=1)
            hit = (h_0_pred.argmax(dim=1) == h0.argmax(dim=1)).float()
            metrics = {phase + ' position error': err.mean(), phase + ' weighted position error': (weight_metric * err).mean(),
                       phase + ' accuracy': hit.mean(), phase + ' weighted accuracy': (weight_metric * hit).mean()}
        return losses, metrics

    sample_lanes = None    # batches that sample() keeps in flight at once (HIP streams / handles); None: 2, or 4 for batches of <= 32
                           # graphs; 1: strictly one after the other
    fused_loss = True      # the losses run as one C-ABI call (pf_train_loss_forward_ep, every parameterisation); False: the framework-op restatement above

    def _loss_tables(self):
        """alpha(gamma(k / T)), sigma(gamma(k / T)) for k = 0..T with the reference's own fp32 expressions (pharmacodiff.py:186-190,
        582-668), on the device: what forward() looks up at t_int."""
        tabs = self.__dict__.get("_loss_tabs")
        if tabs is None or tabs[0].device != self.device:
            t = torch.arange(0, self.n_timesteps + 1, device=self.device).float() / self.n_timesteps
            gamma_t = self.gamma(t)
            tabs = (self.alpha(gamma_t).float().contiguous(), self.sigma(gamma_t).float().contiguous())
            self.__dict__["_loss_tabs"] = tabs
        return tabs

    def _forward_fused(self, g, phase, t_int, eps):
        """forward() through pf_train_loss_forward_ep (endpoint_param_coord / endpoint_param_feat as configured): same draws (t_int, eps), same losses and
        metrics; the pocket's coordinates are the ones bound to the engine (bind_graph), nothing else is uploaded but the
        clean centers."""
        dev = self.device
        dyn = self.dynamics
        eng = dyn.bind_graph(g)
        B = g.batch_size
        x0, h0 = g.pharm_x0.to(dev), g.pharm_h0.to(dev)
        if t_int is None:
            t_int = torch.randint(0, self.n_timesteps, size=(B,), device=dev, dtype=torch.int32)    # (the form the C ABI takes)
        else:
            self._check_injected_t(t_int, B)
        if eps is None:
            eps = {'h': torch.randn(h0.shape, device=dev), 'x': torch.randn(x0.shape, device=dev)}
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p, _, _ in dyn._flat_views)
        p_drop = float(dyn.dropout_rate) if dyn.training else 0.0
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if p_drop > 0 else 0
        args = (x0, h0, t_int, eps['x'], eps['h'], self._loss_tables(), self.n_timesteps, float(self.pharm_feat_norm_constant),
                bool(self.remove_com), bool(self.weighted_loss), p_drop, seed, bool(self.endpoint_param_coord),
                bool(self.endpoint_param_feat))
        if need_grad:
            out, total = _LossFn.apply(dyn, eng, *args, dyn.__dict__["_flat_leaf"])
        else:
            out = eng.train_loss_forward(args[0], args[1], args[2], args[3], args[4], args[5][0], args[5][1], *args[6:10],
                                         dropout=p_drop, seed=seed, ep_coord=args[12], ep_feat=args[13])
            total = out[6]
        losses = {phase + ' pos loss': out[0], phase + ' feat loss': out[1]}
        m = out.detach()
        metrics = {phase + ' position error': m[2], phase + ' weighted position error': m[3],
                   phase + ' accuracy': m[4], phase + ' weighted accuracy': m[5]}
        # the sums a step derives from these (total loss, total error, weighted total error) came out of the same kernel:
        # training_step / validation_step pick them up instead of spending framework launches on three additions
        self.__dict__["_fused_sums"] = (total, m[7], m[8])
        return losses, metrics

    def configure_optimizers(self):
        """pharmacodiff.py:253-263: Adam + ReduceLROnPlateau from lr_scheduler_config."""
        cfg = self.lr_scheduler_config
        optimizer = torch.optim.Adam(self.parameters(), lr=cfg.get('base_lr', 1e-4), weight_decay=cfg.get('weight_decay', 0.0))
        scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, **cfg.get('reducelronplateau', {}))
        return {'optimizer': optimizer,
                'lr_scheduler': {"scheduler": scheduler, "monitor": cfg.get('monitor', 'val total loss'),
                                 "interval": cfg.get('interval', 'step'), "frequency": cfg.get('frequency', 1)}}

    # -- trainer context: Lightning's when attached, else a two-attribute stand-in (attach_trainer) -----------------
    def attach_trainer(self, datamodule, train_dataloader=None, current_epoch: int = 0, optimizer=None):
        """For Lightning-free drivers (train.py here): gives training_step what it reads from ``self.trainer`` in the
        reference -- ``trainer.datamodule.val_dataset`` (pharmacodiff.py:323), ``len(trainer.train_dataloader)``
        (:245) -- plus ``current_epoch`` and the optimiser whose learning rate is logged (:287-290)."""
        from types import SimpleNamespace
        self.__dict__["_pf_trainer"] = SimpleNamespace(datamodule=datamodule, train_dataloader=train_dataloader,
                                                       current_epoch=current_epoch, optimizer=optimizer)

    def _trainer_ctx(self):
        tr = self.__dict__.get("_pf_trainer")
        if tr is not None:
            return tr
        if pl is not None:
            try:
                tr = self.trainer
                from types import SimpleNamespace
                opt = None
                try:
                    opt = self.optimizers()
                except Exception:
                    pass
                return SimpleNamespace(datamodule=tr.datamodule, train_dataloader=tr.train_dataloader,
                                       current_epoch=self.current_epoch, optimizer=opt)
            except Exception:
                return None
        return None

    def num_training_batches(self):
        return len(self._trainer_ctx().train_dataloader)                        # pharmacodiff.py:244-245

    def training_step(self, batch, batch_idx, t_int: torch.Tensor = None, eps: Dict[str, torch.Tensor] = None):
        """pharmacodiff.py:265-296: total loss = pos loss + feat loss (the caller -- Lightning or a plain loop --
        runs .backward() and the optimiser step).  With a trainer context (Lightning's, or attach_trainer) the
        fractional epoch is tracked and, every ``sample_interval`` epochs, sample_and_analyze runs inside the step
        and its metrics join the logged ones (:281-284); without one (a bare loop over tensors) that part is skipped."""
        phase = 'train'
        tr = self._trainer_ctx()
        ph_quality_metrics, epoch_exact = {}, None
        if tr is not None and tr.train_dataloader is not None:
            epoch_exact = tr.current_epoch + batch_idx / max(len(tr.train_dataloader), 1)       # :270
            if epoch_exact - self.last_sample_marker >= self.sample_interval and tr.datamodule is not None:   # :281
                # sampled BEFORE this step's forward (the reference samples between its forward and the caller's
                # backward, :273-284): the engine keeps the activations of one training forward at a time, and sampling
                # rebinds its workspace; the losses / metrics do not depend on the order, only the RNG stream does
                ph_quality_metrics = self.sample_and_analyze()
                self.last_sample_marker = epoch_exact
        loss_dict, metrics_dict = self.forward(batch, phase=phase, t_int=t_int, eps=eps)
        sums = self.__dict__.pop("_fused_sums", None)
        if sums is not None:                       # (the fused loss path computed them with the losses)
            loss_dict[phase + ' total loss'], metrics_dict[phase + ' total error'], metrics_dict[phase + ' weighted total error'] = sums
        else:
            loss_dict[phase + ' total loss'] = torch.sum(torch.stack(list(loss_dict.values()), dim=0))
            metrics_dict[phase + ' total error'] = metrics_dict[phase + ' position error'] + 1 - metrics_dict[phase + ' accuracy']
            metrics_dict[phase + ' weighted total error'] = (metrics_dict[phase + ' weighted position error'] + 1
                                                             - metrics_dict[phase + ' weighted accuracy'])
        metrics_dict.update(ph_quality_metrics)
        if epoch_exact is not None:
            if tr.optimizer is not None:
                metrics_dict['lr'] = tr.optimizer.param_groups[0]['lr']                          # :287-290
            loss_dict['epoch_exact'] = epoch_exact
            self.last_epoch_exact = epoch_exact
        bs = as_pocket_graph(batch).batch_size
        self.log_dict(loss_dict, on_step=True, on_epoch=True, prog_bar=True, logger=True, batch_size=bs)
        self.log_dict(metrics_dict, on_step=True, on_epoch=True, prog_bar=True, logger=True, batch_size=bs)
        self.last_metrics = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in {**loss_dict, **metrics_dict}.items()}
        return loss_dict[phase + ' total loss']

    @torch.no_grad()
    def sample_and_analyze(self, rank: int = 0, world_size: int = 1, process_group=None):
        """pharmacodiff.py:320-357: ``n_pockets_to_sample`` random validation pockets (with replacement, like the
        reference's randint), ``pharms_per_pocket`` pharmacophores each with the reference pharmacophore's size and
        center of mass, batches of 64, validity of the lot."""
        val_dataset = self._trainer_ctx().datamodule.val_dataset
        pocket_idxs = torch.randint(low=0, high=len(val_dataset), size=(self.n_pockets_to_sample,))
        pockets = [val_dataset[int(i)] for i in pocket_idxs]
        return self.sample_and_analyze_graphs(pockets, rank=rank, world_size=world_size, process_group=process_group)

    def validation_step(self, batch, batch_idx):
        phase = 'val'
        loss_dict, metrics_dict = self.forward(batch, phase=phase)
        sums = self.__dict__.pop("_fused_sums", None)
        if sums is not None:
            loss_dict[phase + ' total loss'], metrics_dict[phase + ' total error'], metrics_dict[phase + ' weighted total error'] = sums
        else:
            loss_dict[phase + ' total loss'] = sum(list(loss_dict.values()))
            metrics_dict[phase + ' total error'] = metrics_dict[phase + ' position error'] + 1 - metrics_dict[phase + ' accuracy']
            metrics_dict[phase + ' weighted total error'] = (metrics_dict[phase + ' weighted position error'] + 1
                                                             - metrics_dict[phase + ' weighted accuracy'])
        loss_dict['epoch_exact'] = self.last_epoch_exact
        self.log_dict(loss_dict, on_step=False, on_epoch=True, prog_bar=True, logger=True, batch_size=batch.batch_size)
        self.log_dict(metrics_dict, on_step=False, on_epoch=True, prog_bar=True, logger=True, batch_size=batch.batch_size)
        return loss_dict[phase + ' total loss']

    def sample_and_analyze_graphs(self, pockets: List[PocketGraph], rank=0, world_size=1, process_group=None):
        """sample_and_analyze (pharmacodiff.py:320-357) on explicit pockets; with a process group the
        validity numerator/denominator are summed over ranks with one all-reduce (RCCL on GPUs)."""
        n_pharms = [[g.num_nodes('pharm')] * self.pharms_per_pocket for g in pockets]
        coms = torch.stack([g.pharm_x0.mean(dim=0) for g in pockets], dim=0)
        was_training = self.training
        self.eval()
        sampled = self.sample(pockets, n_pharms, max_batch_size=64, init_pharm_com=coms, rank=rank, world_size=world_size)
        self.train(was_training)
        flat = [p for pocket in sampled for p in pocket]
        return SampleAnalyzer().analyze(flat, process_group=process_group, device=self.device)


def model_from_config(config: dict, ckpt=None) -> PharmacophoreDiff:
    """pharmacoforge/config_utils/load_from_config.py:6-32 (same yaml -> constructor mapping)."""
    ev = config['training']['evaluation']
    return PharmacophoreDiff(
        pharm_nf=len(config['dataset']['ph_type_map']), rec_nf=len(config['dataset']['prot_elements']),
        ph_type_map=config['dataset']['ph_type_map'], processed_data_dir=config['dataset']['processed_data_dir'],
        n_pockets_to_sample=ev['n_pockets'], pharms_per_pocket=ev['pharms_per_pocket'],
        sample_interval=ev['sample_interval'], val_loss_interval=ev['val_loss_interval'],
        batch_size=config['training']['batch_size'], graph_config=config['graph'], dynamics_config=config['dynamics'],
        lr_scheduler_config=config['lr_scheduler'], **config['diffusion'])
