"""GMA attention / aggregation on HIP kernels (reference networks/gma/modules.py).

build_flow_estimator fixes position_only = position_and_content = False and num_heads = 1
(networks/__init__.py:14-19): the content branch.  The two positional variants (modules.py:6-31, 62-68) are built with
RAFTGMA(gma_args(position_only=True)) / RAFTGMA(gma_args(position_and_content=True)): RelPosEmb holds the reference's
tensors (`att.pos_emb.rel_ind`, `.rel_height.weight`, `.rel_width.weight`), and Attention evaluates the two embedding
weights as h + w dot products per query (ops.gma_pos_tables: sim_pos[i, j] = A[i, u] + Bw[i, v]) which the softmax
kernels add to the content logits - or take as the whole logit.  `rel_ind` is never gathered: the kernels index the
weights by u - x + M - 1 themselves.  heads > 1 stays unbuilt.
"""
import torch
import torch.nn as nn

from ... import ops
from .._packs import PackCache, require_cuda


class RelPosEmb(nn.Module):
    def __init__(self, max_pos_size, dim_head):
        super().__init__()
        self.rel_height = nn.Embedding(2 * max_pos_size - 1, dim_head)
        self.rel_width = nn.Embedding(2 * max_pos_size - 1, dim_head)
        idx = torch.arange(max_pos_size)
        self.register_buffer("rel_ind", idx.view(1, -1) - idx.view(-1, 1) + max_pos_size - 1)


class Attention(nn.Module):
    def __init__(self, *, args, dim, max_pos_size=100, heads=4, dim_head=128):
        super().__init__()
        self.args = args
        self.heads = heads
        self.dim_head = dim_head
        self.scale = dim_head ** -0.5
        self.to_qk = nn.Conv2d(dim, heads * dim_head * 2, 1, bias=False)
        self.max_pos_size = max_pos_size
        self.pos_emb = RelPosEmb(max_pos_size, dim_head)
        self._packs = PackCache()

    def _positional(self, fmap):
        """None for the content attention, else whether the content logits take part (position_only wins over
        position_and_content, modules.py:62-68).  Checks what must hold before anything is launched."""
        if self.heads != 1:
            raise NotImplementedError("only the single-head attention is on the AccFlow path")
        if not (self.args.position_only or self.args.position_and_content):
            return None
        h, w = fmap.shape[-2:]
        if h > self.max_pos_size or w > self.max_pos_size:
            raise ValueError("positional attention: the %d x %d feature grid exceeds max_pos_size = %d" % (h, w, self.max_pos_size))
        return not self.args.position_only

    def _tables(self, qk):
        emb = self.pos_emb
        return ops.gma_pos_tables(qk, emb.rel_height.weight.detach().float().contiguous(),
                                  emb.rel_width.weight.detach().float().contiguous(), self.dim_head, self.scale)

    @torch.no_grad()
    def forward(self, fmap):
        """(B, dim, h, w) -> attn (B, heads=1, h*w, h*w) = softmax_j(scale * <q_i, k_j>)  (modules.py:54-76); with
        args.position_and_content the positional logits are added, with args.position_only they are the logits."""
        content = self._positional(fmap)
        require_cuda(fmap)

        def run():
            qk = ops.conv2d(self._packs.conv("qk", self.to_qk), fmap.float())
            if content is not None:
                return ops.gma_attention_pos(qk, self._tables(qk), self.dim_head, self.scale, content)
            return ops.gma_attention(qk, self.dim_head, self.scale)
        return ops.with_range_guard(run, fmap.device, name="%s.forward" % type(self).__name__)

    @torch.no_grad()
    def forward_t(self, fmap, runs=None):
        """Same attention, transposed storage, for Aggregate's matrix-core path (internal to RAFTGMA).  In S16 mode the
        matrix is stored pre-split (ops.gma_attention_s16 / ops.gma_attention_pos_s16): it is the aggregation GEMM's
        activation operand in all 12 refinement iterations and is then never converted again."""
        content = self._positional(fmap)
        require_cuda(fmap)
        qk = ops.conv2d(self._packs.conv("qk", self.to_qk), fmap.float())
        s16 = ops.s16_active() and self.dim_head % 32 == 0
        if content is not None:
            tab = self._tables(qk)
            if s16:
                return TransposedAttention(None, runs, attn16=ops.gma_attention_pos_s16(qk, tab, self.dim_head, self.scale, content))
            return TransposedAttention(ops.gma_attention_pos_t(qk, tab, self.dim_head, self.scale, content), runs)
        if s16:
            return TransposedAttention(None, runs, attn16=ops.gma_attention_s16(qk, self.dim_head, self.scale))
        return TransposedAttention(ops.gma_attention_t(qk, self.dim_head, self.scale), runs)

    @torch.no_grad()
    def forward_alt(self, fmap, runs=None):
        """alternate_attention: no matrix at all - the packs of q and k and the softmax statistics of every query
        (ops.gma_attention_alt, 1 032 bytes per coarse pixel); Aggregate recomputes the probabilities in every refinement
        iteration.  S16 mode only: in fp32 mode, with ACCFLOW_S16=0 and in a range-guard retry (bf16x6) the caller takes
        forward_t / forward, the stored matrix."""
        if self.heads != 1 or self.dim_head != 128 or self.args.position_only or self.args.position_and_content:
            raise NotImplementedError("alternate_attention: only the single-head content attention with dim_head = 128")
        if not ops.s16_active():
            raise RuntimeError("alternate_attention runs in the fp16 split mode with S16 activations only")
        require_cuda(fmap)
        qk = ops.conv2d(self._packs.conv("qk", self.to_qk), fmap.float())
        return TransposedAttention(None, runs, alt=ops.gma_attention_alt(qk, self.dim_head, self.scale))


class TransposedAttention:
    """Hot-path handle: the attention stored j-major (see ops.gma_attention_t)."""

    def __init__(self, attn_t, runs=None, attn16=None, alt=None):
        self.attn_t = attn_t
        self.attn16 = attn16   # ops.S16 (G, P, h, w): the pre-split form (then attn_t is None)
        self.alt = alt         # ops.AltAttention: alternate_attention, no matrix stored (then attn_t and attn16 are None)
        self.runs = runs  # None: attn_t[b] belongs to item b; else [(g, b0, b1)]: items b0..b1-1 all use attn_t[g]


class Aggregate(nn.Module):
    def __init__(self, args, dim, heads=4, dim_head=128):
        super().__init__()
        self.args = args
        self.heads = heads
        self.scale = dim_head ** -0.5
        inner = heads * dim_head
        self.to_v = nn.Conv2d(dim, inner, 1, bias=False)
        self.gamma = nn.Parameter(torch.zeros(1))
        self.project = nn.Conv2d(inner, dim, 1, bias=False) if dim != inner else None
        self._packs = PackCache()

    @torch.no_grad()
    @ops.range_guarded
    def forward(self, attn, fmap, out=None):
        """out = fmap + gamma * (attn @ to_v(fmap))   (modules.py:102-115; project is None for dim == inner)"""
        if self.heads != 1 or self.project is not None:
            raise NotImplementedError("only heads=1, dim == inner_dim is on the AccFlow path")
        fm = fmap.float().contiguous()
        require_cuda(fm)
        v = ops.conv2d(self._packs.conv("v", self.to_v), fm)
        if isinstance(attn, TransposedAttention) and (attn.attn16 is not None or attn.alt is not None):
            if out is None:
                out = torch.empty_like(fm)
            self._aggregate16(attn, v, fm, fm.stride(0), out, None)
            return out
        if isinstance(attn, TransposedAttention):
            if attn.runs is None:
                return ops.gma_aggregate_t(attn.attn_t, v, fm, self.gamma, out=out)
            # items that share one attention matrix are stacked along the output rows of ONE GEMM (the shared
            # matrix is the GEMM's activation operand: read once for the whole run)
            if out is None:
                out = torch.empty_like(fm)
            _, D, h, w = fm.shape
            for g, b0, b1 in attn.runs:
                n = b1 - b0
                if n == 1:
                    ops.gma_aggregate_t(attn.attn_t[g:g + 1], v[b0:b1], fm[b0:b1], self.gamma, out=out[b0:b1])
                else:
                    rows = ops.gma_aggregate_t(attn.attn_t[g:g + 1], v[b0:b1].view(1, n * D, h, w),
                                               fm[b0:b1].view(1, n * D, h, w), self.gamma)
                    out[b0:b1].copy_(rows.view(n, D, h, w))
            return out
        require_cuda(attn)
        return ops.gma_aggregate(attn, v, fm, self.gamma, out=out)

    def _aggregate16(self, attn, v, fmap, fmap_bs, out, out16):
        """One GEMM per run of items sharing an attention matrix; residual read from / results written into the items'
        slices in place (fmap / out: (B, D, h, w) views with any batch stride, out16: ops.S16 or None)."""
        B, D, h, w = v.shape
        runs = attn.runs if attn.runs is not None else [(b, b, b + 1) for b in range(B)]
        if attn.alt is not None:
            for g, b0, b1 in runs:
                ops.gma_aggregate_alt(attn.alt, g, v[b0:b1], fmap[b0].data_ptr(), fmap_bs,
                                      self.gamma, out[b0].data_ptr() if out is not None else None, out.stride(0) if out is not None else 0,
                                      out16.batch(b0, b1).ptr() if out16 is not None else None, out16.bs if out16 is not None else 0,
                                      b1 - b0, D, h, w)
            return
        a16 = attn.attn16
        item = a16.bs * 4
        for g, b0, b1 in runs:
            ops.gma_aggregate_s16(a16.ptr() + g * item, v[b0:b1], fmap[b0].data_ptr(), fmap_bs,
                                  self.gamma, out[b0].data_ptr() if out is not None else None, out.stride(0) if out is not None else 0,
                                  out16.batch(b0, b1).ptr() if out16 is not None else None, out16.bs if out16 is not None else 0,
                                  b1 - b0, D, h, w)

    @torch.no_grad()
    def forward_ws(self, attn, ws, mg32, mg16):
        """Hot path on the update workspace (S16 mode): v from the pre-split motion features, the aggregated features
        straight into the GRU input's fp32 slice mg32 and its S16 form mg16 - no copies, no conversion pass."""
        v = ops.conv2d(self._packs.conv("v", self.to_v), ws.motion16)
        self._aggregate16(attn, v, ws.motion, ws.hx.stride(0), mg32, mg16)
