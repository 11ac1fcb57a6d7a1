"""Attentive-probe evaluation of a frozen DINOv2 backbone on the HIP engine (reference:
dinov2/eval/segmentation/eval_classification.py).

The reference trains a GRID of classifiers on frozen features - learning rates x weight decays per feature source, a
``LinearClassifier`` on every 2-D source (class token, mean patch token, ...) and an ``AttnPoolClassifier`` on every 3-D
source (patch tokens, register tokens) - all of them in every iteration, under one AdamW with a warm-up + cosine schedule,
and keeps the classifier with the best validation accuracy per feature source.

``AttnPoolClassifier`` is one learned query token attending over ``kv = nn.Linear(D, 2D)`` of all tokens.  Because the query
is a single token, keys and values never need to exist (csrc/attnpool.hip): the query is folded through ``Wk`` into one
D-vector per head, the scores of ALL classifiers of a source are one ``[B N, D] x [D, G H]`` product, the tokens are pooled
with the softmax weights BEFORE the value projection, and ``Wv`` is applied to one pooled row per image and head.  It is the
same function, not an approximation; ``fold_forward`` below is the plain-torch statement of it (works on CPU, any dtype).
The classifier linears and the loss of the whole grid run on the probe kernels (csrc/probe.hip): every classifier reads a
column range of ONE feature row ``[2-D sources ... | pooled rows of the 3-D sources ...]``.

Out of scope: datasets, loaders and the 90/10 split, checkpoint files, DDP, torch.compile,
``get_imagenet_class_mapping``, bf16 features.  One GPU."""
import gc
import itertools
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .probe import _HEAD_DTYPE

DEFAULT_LEARNING_RATES = (1e-5, 2e-5, 5e-5, 1e-4, 2e-4, 5e-4, 1e-3, 2e-3, 5e-3, 1e-2)
DEFAULT_WEIGHT_DECAYS = (5e-4, 1e-3, 5e-2)
OBJECT_REPRESENTATIONS = ("avg_objects", "concat_objects", "objects")


# ------------------------------------------------------------------------------------------------ the reference's modules
class LinearClassifier(nn.Module):
    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.linear = nn.Linear(in_dim, out_dim)
        nn.init.trunc_normal_(self.linear.weight, std=0.02)
        nn.init.zeros_(self.linear.bias)

    def forward(self, x):
        return self.linear(x)


class AttnPoolClassifier(nn.Module):
    """forward is the stock composition (kv projection of every token, SDPA); ClassifierGrid runs the folded form."""

    def __init__(self, in_dim, out_dim):
        super().__init__()
        assert in_dim % 64 == 0, f"AttnPoolClassifier: in_dim {in_dim} must be a multiple of 64 (heads of 64)"
        self.num_heads = in_dim // 64
        self.query_token = nn.Parameter(torch.empty(in_dim))
        self.kv = nn.Linear(in_dim, 2 * in_dim)
        self.linear = nn.Linear(in_dim, out_dim)
        for w in (self.query_token, self.kv.weight, self.linear.weight):
            nn.init.trunc_normal_(w, std=0.02)
        nn.init.zeros_(self.kv.bias)
        nn.init.zeros_(self.linear.bias)

    def forward(self, tokens):
        B, N, D = tokens.shape
        H = self.num_heads
        q = self.query_token.expand(B, 1, D).reshape(B, 1, H, 64).transpose(1, 2)
        k, v = self.kv(tokens).reshape(B, N, 2, H, 64).permute(2, 0, 3, 1, 4)
        return self.linear(F.scaled_dot_product_attention(q, k, v).reshape(B, D))


def fold_forward(query_token, kv_weight, kv_bias, tokens):
    """The pooled features [B, D] of an AttnPoolClassifier (the input of its ``linear``) without keys or values - the formulas
    csrc/attnpool.hip runs, in plain torch: u = scale q_h Wk_h per head; p = softmax over tokens of x . u (the key bias is
    constant over tokens and cancels); z = sum_n p x; pooled = Wv_h z + bv_h."""
    B, N, D = tokens.shape
    H = D // 64
    wk, wv, bv = kv_weight[:D], kv_weight[D:], kv_bias[D:]
    u = 0.125 * torch.einsum("hj,hjd->hd", query_token.reshape(H, 64), wk.reshape(H, 64, D))
    p = torch.softmax(torch.einsum("bnd,hd->bnh", tokens, u), dim=1)
    z = torch.einsum("bnh,bnd->bhd", p, tokens)
    return torch.einsum("hjd,bhd->bhj", wv.reshape(H, 64, D), z).reshape(B, D) + bv


class AllClassifiers(nn.ModuleList):
    """The classifiers under keys (feature_source, (lr, wd)), in the dictionary's order; the state dict is the ModuleList's
    (``"{i}.query_token"``, ``"{i}.kv.weight"``, ``"{i}.linear.bias"``, ...), as the reference's ``all_classifiers``."""

    def __init__(self, classifiers):
        self.idx_to_key = list(classifiers.keys())
        super().__init__(classifiers.values())

    def pop_key(self, key):
        i = self.idx_to_key.index(key)
        self.idx_to_key.pop(i)
        return self.pop(i)

    def forward(self, backbone_out):
        return {key: self[i](backbone_out[key[0]]) for i, key in enumerate(self.idx_to_key)}

    def load_state_dict(self, sd, strict=True, **kw):
        """Also takes the state of the reference's DDP wrapper (``module.`` in front of every key)."""
        sd = OrderedDict(((k[len("module."):] if k.startswith("module.") else k), v) for k, v in sd.items())
        return super().load_state_dict(sd, strict=strict, **kw)


class AnyMatchAccuracy:
    """A prediction counts when one of the top_k classes is among the sample's targets; targets are padded with -1, and a
    sample without any valid target is left out of the mean.  preds [n_head, n_cls, bs], target [n_head, bs, n_annot] (the
    heads share the targets; the first head's are used)."""

    def __init__(self, top_k=1):
        self.top_k = int(top_k)
        self.reset()

    def reset(self):
        self.tp, self.count = None, None

    def update(self, preds, target):
        top = preds.topk(self.top_k, dim=1).indices                  # [n_head, k, bs]
        t = target[0].long()                                         # [bs, n_annot]
        valid = t >= 0
        hit = ((top[..., None] == t[None, None]) & valid[None, None]).any(-1).any(1)     # [n_head, bs]
        keep = valid.any(-1)
        tp, n = (hit & keep[None]).sum(1), keep.sum()
        self.tp = tp if self.tp is None else self.tp + tp
        self.count = n if self.count is None else self.count + n

    def compute(self):
        return self.tp.float() / self.count.float()


# ------------------------------------------------------------------------------------------------ features
def feature_sources(representations, embed_dim, num_register_tokens):
    """name -> (ndim, width) of the BackboneWrapper dictionary, in its order.  ``cls_avg_patch`` is always there: the
    reference tests the string itself (``if "cls_avg_patch":``), which is always true."""
    D, R = int(embed_dim), int(num_register_tokens)
    if not R and any(r in representations for r in OBJECT_REPRESENTATIONS):
        raise ValueError("classification: the objects representations need a model with register tokens")
    out = OrderedDict()
    if "cls" in representations:
        out["cls"] = (2, D)
    if "avg_patch" in representations:
        out["avg_patch"] = (2, D)
    out["cls_avg_patch"] = (2, 2 * D)
    if "avg_objects" in representations:
        out["avg_objects"] = (2, D)
    if "concat_objects" in representations:
        out["concat_objects"] = (2, R * D)
    if "objects" in representations:
        out["reg"] = (3, D)
    if "patch" in representations:
        out["patch"] = (3, D)
    return out


@torch.no_grad()
def features(model, images, representations):
    """The BackboneWrapper dictionary from the model's last-layer tokens (``forward_features``); patch tokens in float32."""
    out_tokens = model.forward_features(images)
    cls, reg = out_tokens["x_norm_clstoken"], out_tokens["x_norm_regtokens"]
    patch = out_tokens["x_norm_patchtokens"].float()
    if reg.shape[1] == 0 and any(r in representations for r in OBJECT_REPRESENTATIONS):
        raise ValueError("classification: the objects representations need a model with register tokens")
    out = OrderedDict()
    if "cls" in representations:
        out["cls"] = cls
    if "avg_patch" in representations:
        out["avg_patch"] = patch.mean(1)
    out["cls_avg_patch"] = torch.cat([cls, patch.mean(1)], dim=-1)
    if "avg_objects" in representations:
        out["avg_objects"] = reg.mean(1)
    if "concat_objects" in representations:
        out["concat_objects"] = reg.flatten(1, 2)
    if "objects" in representations:
        out["reg"] = reg
    if "patch" in representations:
        out["patch"] = patch
    return out


def lr_schedule(n_iters, warmup_iters):
    warmup = np.linspace(0.0, 1.0, warmup_iters)
    decay = (np.cos(np.linspace(0, np.pi, n_iters - warmup_iters)) + 1) / 2
    return np.concatenate([warmup, decay])


def best_keys(keys, accuracies):
    """feature source -> its key with the highest accuracy, the first one on ties (what ``idxmax`` gives)."""
    best = OrderedDict()
    for key, acc in zip(keys, accuracies):
        if key[0] not in best or acc > best[key[0]][1]:
            best[key[0]] = (key, acc)
    return OrderedDict((s, k) for s, (k, _) in best.items())


# ------------------------------------------------------------------------------------------------ the grid
class _Source:
    """The classifiers of one feature source: positions i0 .. i0 + G - 1 of the grid, columns col0 .. of the feature row."""

    def __init__(self, name, attn, K, i0, G, col0):
        self.name, self.attn, self.K, self.i0, self.G, self.col0 = name, attn, K, i0, G, col0
        self.cap = 0


class ClassifierGrid:
    """The classifier grid of eval_classification.py on top of ``model`` (anything with ``forward_features``, ``embed_dim``
    and ``num_register_tokens``; ``model=None`` with ``embed_dim=`` / ``num_register_tokens=`` for a grid on resident features).

    ``classifiers`` is an ``AllClassifiers`` of the reference's modules whose parameters are views of one flat f32 buffer
    (``flat``; gradients in ``grad_flat``, AdamW moments in the optimizer's flat buffers): ``classifiers.state_dict()`` /
    ``load_state_dict`` move checkpoints of the reference's ``all_classifiers`` both ways, and ``classifiers(feats)`` is the
    stock forward on the same weights.  ``step`` never synchronises with the host."""

    def __init__(self, model, representations=("cls", "avg_patch", "patch"), learning_rates=DEFAULT_LEARNING_RATES,
                 weight_decays=DEFAULT_WEIGHT_DECAYS, batch_size=128, num_classes=1000, n_iters=12500, warmup_iters=1250,
                 world_size=1, device=None, embed_dim=None, num_register_tokens=None):
        self.model = model
        self.representations = tuple(representations)
        self.batch_size, self.num_classes = int(batch_size), int(num_classes)
        D = self.embed_dim = int(model.embed_dim if model is not None else embed_dim)
        R = int(getattr(model, "num_register_tokens", 0) if model is not None else (num_register_tokens or 0))
        shapes = feature_sources(self.representations, D, R)
        if D % 64:
            raise ValueError(f"ClassifierGrid: embed_dim {D} must be a multiple of 64")
        self.n_iters, self.warmup_iters = int(n_iters), int(warmup_iters)
        self.schedule = lr_schedule(self.n_iters, self.warmup_iters)
        self.iteration = 0
        if device is None:
            device = next(model.parameters()).device if model is not None else torch.device("cpu")
        self.device = torch.device(device)
        classifiers, self.hyper = OrderedDict(), {}
        for source, (ndim, width) in shapes.items():
            cls = LinearClassifier if ndim == 2 else AttnPoolClassifier
            for lr, wd in itertools.product(learning_rates, weight_decays):
                key = (source, (lr, wd))
                classifiers[key] = cls(width, self.num_classes)
                self.hyper[key] = (lr * (self.batch_size * world_size) / 256.0, wd)
        self.classifiers = AllClassifiers(classifiers)
        self.optimizer = None
        self._table = None
        self._adopt()
        if self.device.type == "cuda":
            self._rebuild()

    def __len__(self):
        return len(self.classifiers)

    @property
    def keys(self):
        return list(self.classifiers.idx_to_key)

    def param_hyper(self):
        """(name, base_lr, weight_decay) of every parameter in the classifiers' order: the reference's grouping - no decay
        for a parameter whose name contains "bias", wd for the rest (the query token included)."""
        out = []
        for i, key in enumerate(self.classifiers.idx_to_key):
            base_lr, wd = self.hyper[key]
            for name, _ in self.classifiers[i].named_parameters():
                out.append((f"{i}.{name}", base_lr, 0.0 if "bias" in name else wd))
        return out

    # ------------------------------------------------------------------------------------------ storage
    def _adopt(self):
        """Move every parameter into one flat buffer on the device (each tensor 16-byte aligned) and give it a gradient view."""
        params = list(self.classifiers.parameters())
        total = sum((p.numel() + 3) // 4 * 4 for p in params)
        self.flat = torch.zeros(total, dtype=torch.float32, device=self.device)
        self.grad_flat = torch.zeros(total, dtype=torch.float32, device=self.device)
        off = 0
        for p in params:
            n = p.numel()
            view = self.flat[off:off + n].view(p.shape)
            view.copy_(p.data)
            p.data = view
            p.grad = self.grad_flat[off:off + n].view(p.shape)
            off += (n + 3) // 4 * 4

    def _need_gpu(self):
        if self._table is None:
            raise RuntimeError("ClassifierGrid: the classifier kernels run on the GPU only (no CPU fallback)")

    def _rebuild(self):
        """Everything derived from the classifier list: sources, the feature-row layout, the device tables, the optimizer."""
        from . import ops
        from .train import FusedLamb
        dev = self.device
        self.sources, col0 = [], 0
        for i, (name, _) in enumerate(self.classifiers.idx_to_key):
            if self.sources and self.sources[-1].name == name:
                self.sources[-1].G += 1
                continue
            if any(s.name == name for s in self.sources):
                raise RuntimeError("ClassifierGrid: the classifiers of a feature source must be adjacent")
            m = self.classifiers[i]
            if self.sources:
                last = self.sources[-1]
                col0 = last.col0 + (last.G * last.K if last.attn else last.K)
            self.sources.append(_Source(name, isinstance(m, AttnPoolClassifier), m.linear.in_features, i, 1, col0))
        last = self.sources[-1]
        self.width = last.col0 + (last.G * last.K if last.attn else last.K)
        nh = len(self.classifiers)
        tab = np.zeros(nh, dtype=_HEAD_DTYPE)
        tile0 = 0
        for s in self.sources:
            mods = [self.classifiers[s.i0 + g] for g in range(s.G)]
            for g, m in enumerate(mods):
                tab[s.i0 + g] = (m.linear.weight.data_ptr(), m.linear.bias.data_ptr(), 0, 0,
                                 s.col0 + (g * s.K if s.attn else 0), s.K, s.i0 + g, tile0)
                tile0 += s.K // 64
            T = lambda ts: ops.ptr_table(ts, dev)
            s.w, s.dw = T([m.linear.weight for m in mods]), T([m.linear.weight.grad for m in mods])
            s.db = T([m.linear.bias.grad for m in mods])
            if s.attn:
                D = s.K
                s.q, s.dq = T([m.query_token for m in mods]), T([m.query_token.grad for m in mods])
                s.wk, s.dwk = T([m.kv.weight for m in mods]), T([m.kv.weight.grad for m in mods])
                s.wv, s.dwv = T([m.kv.weight[D:] for m in mods]), T([m.kv.weight.grad[D:] for m in mods])
                s.bv, s.dbk = T([m.kv.bias[D:] for m in mods]), T([m.kv.bias.grad[:D] for m in mods])
                s.dbv = T([m.kv.bias.grad[D:] for m in mods])
            # one table per source: its logits start at a 16-byte aligned offset of the logits buffer (_offsets)
            s.table = torch.from_numpy(tab[s.i0:s.i0 + s.G].copy().view(np.uint8)).to(dev)
        self._table = [s.table for s in self.sources]
        self.loss = torch.zeros(nh, dtype=torch.float32, device=dev)            # per-classifier batch mean
        self._cap = 0
        self._reserve(self.batch_size)
        groups = []
        for i, key in enumerate(self.classifiers.idx_to_key):
            base_lr, wd = self.hyper[key]
            named = list(self.classifiers[i].named_parameters())
            groups.append({"params": [p for n, p in named if "bias" not in n], "lr": 0.0, "weight_decay": wd, "base_lr": base_lr})
            groups.append({"params": [p for n, p in named if "bias" in n], "lr": 0.0, "weight_decay": 0.0, "base_lr": base_lr})
        self.optimizer = FusedLamb(groups, lr=0.0, betas=(0.9, 0.95), eps=1e-8, max_grad_norm=0.0, adam=True)

    def _reserve(self, B):
        if B <= self._cap:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ClassifierGrid: a batch larger than the reserved buffers during graph capture")
        nh, C, dev = len(self.classifiers), self.num_classes, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.features = torch.zeros(B, self.width, **f32)
        self._dfeatures = torch.zeros(B, self.width, **f32)
        total = self._offsets(B)[-1]
        self._logits = torch.empty(total, **f32)
        self._dlogits = torch.empty(total, **f32)
        self._rowloss = torch.empty(nh * B, **f32)
        self._rowrank = torch.empty(nh * B, dtype=torch.int32, device=dev)
        self._cap = B

    def _reserve_tokens(self, s, B, N):
        from ._lib import DENSE_F32_TN, check, lib
        D = s.K
        GH = s.G * (D // 64)
        GHp = (GH + 3) // 4 * 4
        need = int(lib().octic_dense_f32_workspace_bytes(DENSE_F32_TN, B * N, GHp, D))
        if need < 0:
            check(need)
        if B * N <= s.cap and B <= s.cap_b and need <= s.ws.numel():
            return GH, GHp
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ClassifierGrid: token buffers cannot grow during graph capture")
        f32 = dict(dtype=torch.float32, device=self.device)
        s.U, s.dU = torch.zeros(GHp, D, **f32), torch.zeros(GHp, D, **f32)
        s.S, s.dS = torch.empty(B * N * GHp, **f32), torch.empty(B * N * GHp, **f32)
        s.Z, s.dZ = torch.empty(B * GH * D, **f32), torch.empty(B * GH * D, **f32)
        s.ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        s.cap, s.cap_b = B * N, B
        return GH, GHp

    def _offsets(self, B):
        """Where each source's [G, B, C] block starts in the logits buffers (16-byte aligned), and the total length."""
        offs = [0]
        for s in self.sources:
            offs.append(offs[-1] + (s.G * B * self.num_classes + 3) // 4 * 4)
        return offs

    def _blocks(self, buf, B):
        C = self.num_classes
        return [buf[o:o + s.G * B * C] for s, o in zip(self.sources, self._offsets(B))]

    def logits(self, B):
        """The last forward's logits as [classifiers, B, C] (a copy where the grid has more than one feature source)."""
        blocks = [b.view(-1, B, self.num_classes) for b in self._blocks(self._logits, B)]
        return blocks[0] if len(blocks) == 1 else torch.cat(blocks)

    # ------------------------------------------------------------------------------------------ stages
    def extract(self, images):
        """Frozen backbone in eval mode -> the feature dictionary."""
        self._need_gpu()
        if self.model is None:
            raise RuntimeError("ClassifierGrid: built without a backbone (features only)")
        self.model.eval()
        return features(self.model, images, self.representations)

    @staticmethod
    def _token_rows(x, D):
        """[B, N, D] f32 tokens as rows the kernels take: unit channel stride, one 16-byte aligned row stride over all B N rows."""
        B, N, _ = x.shape
        ldx = x.stride(1)
        if not (x.stride(2) == 1 and x.data_ptr() % 16 == 0 and ldx % 4 == 0 and ldx >= D and x.stride(0) == N * ldx):
            x, ldx = x.contiguous(), D
        return x, ldx

    def forward_features(self, feats):
        """All classifiers on a feature dictionary: logits [classifiers, B, C] (a view, overwritten by the next call)."""
        from . import ops
        self._need_gpu()
        first = feats[self.sources[0].name]
        if not first.is_cuda:
            raise RuntimeError("ClassifierGrid: features must be CUDA tensors (the classifier kernels run on the GPU only)")
        B = first.shape[0]
        self._reserve(B)
        Frow = self.features[:B]
        self._saved = []
        for s in self.sources:
            x = feats[s.name]
            if x.shape[0] != B or x.shape[-1] != s.K or x.dim() != (3 if s.attn else 2):
                raise ValueError(f"ClassifierGrid: feature {s.name!r} has shape {tuple(x.shape)}, expected width {s.K}")
            if not s.attn:
                Frow[:, s.col0:s.col0 + s.K].copy_(x)
                continue
            if x.dtype != torch.float32:
                raise TypeError("ClassifierGrid: token features must be float32 (bf16 features are not supported)")
            D, N = s.K, x.shape[1]
            x, ldx = self._token_rows(x, D)
            GH, GHp = self._reserve_tokens(s, B, N)
            X2 = x.as_strided((B * N, D), (ldx, 1))
            S = s.S[:B * N * GHp].view(B * N, GHp)
            Z = s.Z[:B * GH * D]
            ops.attnpool_fold(s.q, s.wk, s.G, D, s.U)
            ops.dense_f32_nt(X2, s.U, out=S, name="attnpool_scores<dense_f32_nt>")
            ops.attnpool_softmax(S, B, N, GH)
            ops.attnpool_pool(S, x, ldx, B, N, D, GH, Z)
            ops.attnpool_value(Z, s.wv, s.bv, B, s.G, D, Frow[:, s.col0:])
            self._saved.append((s, x, ldx, X2, S, Z, N, GH, GHp))
        for s, block in zip(self.sources, self._blocks(self._logits, B)):
            ops.probe_forward(s.table, s.G, Frow, B, self.num_classes, block, s.G * s.K)
        self._last_B = B
        return self.logits(B)

    def pooled(self, source, B):
        """The last forward's pooled rows [B, G, D] of an attention-pooling source (a view of the feature row)."""
        s = next(t for t in self.sources if t.name == source and t.attn)
        return self.features[:B, s.col0:s.col0 + s.G * s.K].view(B, s.G, s.K)

    def backward(self, labels):
        """Cross entropy of the last logits (``self.loss``: batch means per classifier) and every parameter gradient of
        mean-over-batch-and-classifiers of it, written into ``grad_flat``."""
        from . import ops
        B, C, nh = self._last_B, self.num_classes, len(self.classifiers)
        dlogits = self._blocks(self._dlogits, B)
        for s, lg, dl in zip(self.sources, self._blocks(self._logits, B), dlogits):
            ops.probe_ce(lg, labels, s.G, B, C, dl, self._rowloss[s.i0 * B:], self._rowrank[s.i0 * B:],
                         loss_mean=self.loss[s.i0:s.i0 + s.G])
        alpha = 1.0 / nh                                   # octic_probe_ce gives 1 / B; the mean over classifiers rides here
        Frow, dF = self.features[:B], self._dfeatures[:B]
        saved = {id(t[0]): t for t in self._saved}
        for s, dl in zip(self.sources, dlogits):
            ops.attnpool_colsum(dl, B * C, C, s.G, B, C, alpha, s.db)
            ops.attnpool_dweight(dl, Frow, s.col0, s.K if s.attn else 0, s.G, B, C, s.K, alpha, s.dw)
            if not s.attn:
                continue
            _, x, ldx, X2, S, Z, N, GH, GHp = saved[id(s)]
            D = s.K
            dP = dF[:, s.col0:]
            ops.attnpool_dinput(dl, s.w, s.G, B, C, D, alpha, dP)
            ops.attnpool_colsum(dP, D, dF.stride(0), s.G, B, D, 1.0, s.dbv)
            dZ = s.dZ[:B * GH * D]
            ops.attnpool_dz(dP, s.wv, B, s.G, D, dZ)
            ops.attnpool_dwv(dP, Z, B, s.G, D, s.dwv)
            dS = s.dS[:B * N * GHp].view(B * N, GHp)
            ops.attnpool_dscores(x, ldx, dZ, S, B, N, D, GH, dS)
            ops.dense_f32_tn(dS, X2, out=s.dU, workspace=s.ws, name="attnpool_dfold<dense_f32_tn>")
            ops.attnpool_unfold(s.q, s.wk, s.dU, s.G, D, s.dq, s.dwk, s.dbk)

    def _set_lr(self):
        f = float(self.schedule[min(self.iteration, len(self.schedule) - 1)])
        for g in self.optimizer.param_groups:
            g["lr"] = f * g["base_lr"]

    def _check_labels(self, labels, B):
        if not labels.is_cuda:
            raise RuntimeError("ClassifierGrid: labels must be a CUDA tensor (the classifier kernels run on the GPU only)")
        if labels.dtype != torch.int64 or labels.shape != (B,):
            raise ValueError("ClassifierGrid.step: labels must be int64 [B] class indices")

    def step_features(self, feats, labels):
        """One training iteration on a feature dictionary: forward, cross entropy, backward, AdamW under the schedule.
        Returns the per-classifier losses (device tensor, overwritten by the next step; their mean is the reference's loss)."""
        self._need_gpu()
        self.forward_features(feats)
        self._check_labels(labels, self._last_B)
        self.backward(labels)
        self._set_lr()
        self.optimizer.step()
        self.iteration += 1
        return self.loss

    def step(self, images, labels):
        if not images.is_cuda:
            raise RuntimeError("ClassifierGrid: images must be a CUDA tensor (the classifier kernels run on the GPU only)")
        return self.step_features(self.extract(images), labels)

    def capture(self, example_images, example_labels, warmup=2):
        """Record ``step`` once as a hipGraph; returns a callable ``replay(images, labels)``."""
        return CapturedGridStep(self, example_images, example_labels, warmup)

    # ------------------------------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def evaluate(self, batches, on_features=False):
        """AnyMatchAccuracy (top-1) of every classifier over ``batches`` of (images | feature dictionary, labels); labels
        [B] or [B, n_annot] padded with -1.  One read-back at the end.  Returns {"accuracy": {key: acc}, "best": {feature
        source: key}, "samples": n}."""
        self._need_gpu()
        metric = AnyMatchAccuracy(top_k=1)
        nh = len(self.classifiers)
        for x, labels in batches:
            logits = self.forward_features(x if on_features else self.extract(x))
            t = labels.to(logits.device)
            t = t[:, None] if t.dim() == 1 else t
            metric.update(logits.permute(0, 2, 1), t[None].expand(nh, -1, -1))
        acc = metric.compute().cpu().tolist()
        keys = self.keys
        return {"accuracy": OrderedDict(zip(keys, acc)), "best": best_keys(keys, acc), "samples": int(metric.count.item())}

    def keep_best(self, val_metrics):
        """Drop every classifier that is not the best of its feature source (the optimizer state goes with them: the
        reference deletes its optimizer before this point)."""
        keep = set(val_metrics["best"].values())
        for key in [k for k in self.classifiers.idx_to_key if k not in keep]:
            self.classifiers.pop_key(key)
        if self.device.type == "cuda":
            self._rebuild()

    def state_dict(self):
        return self.classifiers.state_dict()

    def load_state_dict(self, sd):
        return self.classifiers.load_state_dict(sd)


class CapturedGridStep:
    """``ClassifierGrid.step`` as one hipGraph replay (static shapes): images and labels are copied into the graph's inputs,
    the iteration's learning rates into the device buffer the AdamW kernels read."""

    def __init__(self, grid, images, labels, warmup=2):
        if not images.is_cuda:
            raise RuntimeError("CapturedGridStep: CUDA example inputs are required")
        self.grid = grid
        self.images, self.labels = images.detach().clone(), labels.detach().clone()
        dev = images.device
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(max(1, warmup)):       # fills the backbone's caches and sizes the buffers; no parameter changes
                grid.forward_features(grid.extract(self.images))
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        it, count = grid.iteration, grid.optimizer.step_count
        grid._set_lr()
        grid.optimizer.prepare_capture()
        gc.collect()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss = grid.step(self.images, self.labels)
        grid.iteration, grid.optimizer.step_count = it, count      # the capture ran nothing

    def __call__(self, images, labels):
        if images.shape != self.images.shape or images.dtype != self.images.dtype or labels.shape != self.labels.shape:
            raise ValueError("CapturedGridStep: inputs differ in shape or dtype from the captured ones")
        g = self.grid
        self.images.copy_(images, non_blocking=True)
        self.labels.copy_(labels, non_blocking=True)
        g._set_lr()
        g.optimizer.push_hyper()
        self.graph.replay()
        g.iteration += 1
        g.optimizer.step_count += 1
        return self.loss

    replay = __call__


def eval_model(model, train_batches, val_batches, test_batches_by_name, **grid_kwargs):
    """eval_classification.eval_model on batches the caller provides: train the grid for ``n_iters`` iterations over
    ``train_batches`` (an iterable of (images, labels), restarted when it ends), pick the best classifier per feature source
    on ``val_batches``, drop the rest, and evaluate the survivors on every test set.  Returns
    {"{feature_source}_{test_name}_acc": accuracy}."""
    grid = ClassifierGrid(model, **grid_kwargs)
    while grid.iteration < grid.n_iters:
        n0 = grid.iteration
        for images, labels in train_batches:
            if grid.iteration >= grid.n_iters:
                break
            grid.step(images, labels)
        if grid.iteration == n0:
            raise ValueError("eval_model: train_batches is empty")
    grid.keep_best(grid.evaluate(val_batches))
    results = OrderedDict()
    for name, batches in test_batches_by_name.items():
        for (source, _), acc in grid.evaluate(batches)["accuracy"].items():
            results[f"{source}_{name}_acc"] = acc
    return results
