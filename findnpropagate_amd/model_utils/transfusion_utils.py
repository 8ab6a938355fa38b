"""pcdet/models/model_utils/transfusion_utils.py with the reference's signatures: clip_sigmoid (:5-7), PositionEmbeddingLearned
(:10-26) and TransformerDecoderLayer (:29-101).  The modules keep the reference's submodule and parameter names, so a
reference checkpoint's `decoder.*` keys load with strict=True.

TransformerDecoderLayer.forward runs on the library's kernels (csrc/tfdecoder.hip, seven launches, eight with more than 256 queries, nothing read on the host)
when plain_reasons() finds nothing against it; otherwise it is forward_plain, the reference's own torch ops with dropout and
gradients, so training is unchanged.  With the attribute fused_attention_grad set (default off) the cross attention's core runs
on the library's differentiable kernels there (forward_fused_grad) whenever fused_grad_reasons() finds nothing against it."""
import torch
import torch.nn.functional as F
from torch import nn


def clip_sigmoid(x, eps=1e-4):
    """clamp(sigmoid(x), eps, 1 - eps).  As in the reference the sigmoid is taken IN PLACE: x holds sigmoid(x) afterwards.
    utils.loss_utils.heatmap_loss, the fused path, leaves its logits alone."""
    y = torch.clamp(x.sigmoid_(), min=eps, max=1 - eps)
    return y


class PositionEmbeddingLearned(nn.Module):
    """Learned absolute position embedding: positions (B, P, input_channel) -> (B, num_pos_feats, P) through
    Conv1d, BatchNorm1d, ReLU, Conv1d (1-wide), held as `position_embedding_head`."""

    def __init__(self, input_channel, num_pos_feats=288):
        super().__init__()
        layers = [nn.Conv1d(input_channel, num_pos_feats, 1), nn.BatchNorm1d(num_pos_feats), nn.ReLU(inplace=True),
                  nn.Conv1d(num_pos_feats, num_pos_feats, 1)]
        self.position_embedding_head = nn.Sequential(*layers)

    def forward(self, xyz):
        return self.position_embedding_head(xyz.transpose(1, 2).contiguous())


_ACTIVATIONS = {"relu": F.relu, "gelu": F.gelu, "glu": F.glu}


def _rows(t):
    """(B, C, P) -> (P, B, C): nn.MultiheadAttention's sequence-first layout"""
    return t.permute(2, 0, 1)


class TransformerDecoderLayer(nn.Module):
    """One post-norm decoder layer over channel-major maps: self-attention among the queries (unless cross_only), cross
    attention of the queries over the keys, an FFN; each followed by dropout, the residual and a LayerNorm; the position
    embeddings are added to the attention inputs (queries, keys AND values, as the reference does), not to the residual.

    forward(query (B, C, Pq), key (B, C, Pk), query_pos (B, Pq, 2), key_pos (B, Pk, 2)) -> (B, C, Pq).  Submodules carry the
    reference's names and are created in its order (so a seeded construction draws the same numbers)."""

    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, activation="relu",
                 self_posembed=None, cross_posembed=None, cross_only=False):
        super().__init__()
        if activation not in _ACTIVATIONS:
            raise RuntimeError(f"activation should be relu/gelu, not {activation}.")
        self.cross_only = cross_only
        if not cross_only:
            self.self_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)
        self.multihead_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)
        self.linear1, self.dropout = nn.Linear(d_model, dim_feedforward), nn.Dropout(dropout)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        for i in (1, 2, 3):
            setattr(self, f"norm{i}", nn.LayerNorm(d_model))
        for i in (1, 2, 3):
            setattr(self, f"dropout{i}", nn.Dropout(dropout))
        self.activation_name, self.activation = activation, _ACTIVATIONS[activation]
        self.self_posembed, self.cross_posembed = self_posembed, cross_posembed
        self._device_pack = None      # the device path's cached state (dense_heads.transfusion_decoder.DevicePack), made on first use

    def __getstate__(self):
        """copies, pickles and saved modules travel without the device path's cache (packed weights, the key position
        embedding, a ctypes array): it is rebuilt on first use"""
        state = dict(self.__dict__)
        state["_device_pack"] = None
        return state

    def with_pos_embed(self, tensor, pos_embed):
        return tensor if pos_embed is None else tensor + pos_embed

    def plain_reasons(self, query, key, query_pos, key_pos, key_padding_mask=None, attn_mask=None):
        """what stands against the device path, as a list of short strings (empty: the device path runs)"""
        from ..dense_heads.transfusion_decoder import DevicePack

        if self._device_pack is None:
            self._device_pack = DevicePack(self, None)
        return self._device_pack.reasons(query, key, query_pos, key_pos, key_padding_mask, attn_mask)

    # Opt-in: under autograd or in train(), where the eval device path does not apply, run the cross attention's core
    # softmax(0.25 q.k) v on the library's differentiable kernels (dense_heads.transfusion_decoder.attention_autograd) instead
    # of materialising the 8 x Pq x Pk scores.  A plain attribute: not a constructor argument, not in the state_dict.
    fused_attention_grad = False
    # Opt-in on top of fused_attention_grad: in train() with multihead_attn.dropout > 0 the fused route applies that dropout
    # inside the kernels (a counter-based mask from a freshly drawn seed, regenerated in the backward; include/fnp.h), where
    # forward_plain draws torch's mask: the same distribution, other bits.  A plain attribute like the one above.
    fused_attention_dropout = False

    def fused_grad_reasons(self, query, key, query_pos, key_pos, key_padding_mask=None, attn_mask=None):
        """what stands against forward_fused_grad, as a list of short strings (empty: it can run).  A layer in train() with
        multihead_attn.dropout > 0 keeps forward_plain unless fused_attention_dropout is set."""
        from ..dense_heads.transfusion_decoder import D_MODEL, MAX_QUERIES, N_HEAD

        r = []
        if key_padding_mask is not None or attn_mask is not None:
            r.append("mask")
        mha = self.multihead_attn
        if mha.embed_dim != D_MODEL or mha.num_heads != N_HEAD or mha.in_proj_weight is None or mha.in_proj_bias is None:
            r.append("d_model / nhead")
        if self.training and mha.dropout != 0 and not (self.fused_attention_dropout and 0 < mha.dropout < 1):
            r.append("attention dropout")
        tensors = [query, key, query_pos, key_pos] + list(self.parameters()) + [b for b in self.buffers() if b.is_floating_point()]
        if any(t.dtype != torch.float32 for t in tensors):
            r.append("dtype")
        if not all(t.is_cuda for t in tensors) or len({t.device for t in tensors}) > 1:
            r.append("not on the device")
        if not r:
            ok = query.dim() == 3 and key.dim() == 3 and query.shape[1] == D_MODEL and key.shape[:2] == (query.shape[0], D_MODEL)
            if not (ok and 1 <= query.shape[2] <= MAX_QUERIES and 1 <= key.shape[2] < 2 ** 31 // D_MODEL):
                r.append("shape")
        return r

    def forward(self, query, key, query_pos, key_pos, key_padding_mask=None, attn_mask=None):
        reasons = self.plain_reasons(query, key, query_pos, key_pos, key_padding_mask, attn_mask)
        if reasons:
            wanted = self.fused_attention_grad and ("autograd" in reasons or "training mode" in reasons)
            if wanted and not self.fused_grad_reasons(query, key, query_pos, key_pos, key_padding_mask, attn_mask):
                return self.forward_fused_grad(query, key, query_pos, key_pos)
            return self.forward_plain(query, key, query_pos, key_pos, key_padding_mask, attn_mask)
        return self._device_pack.run(query, key, query_pos, key_pos)[0]

    def forward_plain(self, query, key, query_pos, key_pos, key_padding_mask=None, attn_mask=None):
        """the layer as torch ops, differentiable, with dropout in train(): what forward runs off the device path"""
        return self._forward_torch(query, key, query_pos, key_pos, key_padding_mask, attn_mask, self._cross_plain)

    def forward_fused_grad(self, query, key, query_pos, key_pos):
        """forward_plain with the cross attention's core on the differentiable kernels: the in- and out-projections stay
        F.linear, everything else the same torch ops in the same order.  No masks; attention dropout in train() only with
        fused_attention_dropout, inside the kernels (fused_grad_reasons)."""
        return self._forward_torch(query, key, query_pos, key_pos, None, None, self._cross_fused)

    def _cross_plain(self, q_in, m, key_padding_mask, attn_mask):
        return self.multihead_attn(query=q_in, key=m, value=m, key_padding_mask=key_padding_mask, attn_mask=attn_mask)[0]

    def _cross_fused(self, q_in, m, key_padding_mask, attn_mask):
        """nn.MultiheadAttention(q_in (Pq, B, C), m, m)[0] without masks, on (B, L, 128) rows; its dropout on the probabilities
        (train() only) runs inside the kernels, on a seed drawn here"""
        from ..dense_heads import transfusion_decoder as TD

        mha = self.multihead_attn
        p = mha.dropout if self.training and self.fused_attention_dropout else 0.0
        w, b, d = mha.in_proj_weight, mha.in_proj_bias, mha.embed_dim
        rows_q, rows_m = q_in.transpose(0, 1), m.transpose(0, 1)
        q = F.linear(rows_q, w[:d], b[:d])
        k = F.linear(rows_m, w[d:2 * d], b[d:2 * d])
        v = F.linear(rows_m, w[2 * d:], b[2 * d:])
        core = TD.attention_autograd(q, k, v, p, TD.draw_dropout_seed(q.device)) if p > 0 else TD.attention_autograd(q, k, v)
        return F.linear(core, mha.out_proj.weight, mha.out_proj.bias).transpose(0, 1)

    def _forward_torch(self, query, key, query_pos, key_pos, key_padding_mask, attn_mask, cross):
        q_pe = None if self.self_posembed is None else _rows(self.self_posembed(query_pos))
        k_pe = None if self.cross_posembed is None else _rows(self.cross_posembed(key_pos))
        x, memory = _rows(query), _rows(key)
        if not self.cross_only:
            a = self.with_pos_embed(x, q_pe)
            x = self.norm1(x + self.dropout1(self.self_attn(a, a, value=a)[0]))
        m = self.with_pos_embed(memory, k_pe)
        attended = cross(self.with_pos_embed(x, q_pe), m, key_padding_mask, attn_mask)
        x = self.norm2(x + self.dropout2(attended))
        x = self.norm3(x + self.dropout3(self.linear2(self.dropout(self.activation(self.linear1(x))))))
        return x.permute(1, 2, 0)
