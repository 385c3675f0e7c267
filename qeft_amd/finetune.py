"""The training step the project is named after: a causal-LM loss over a packed model whose only trainable parameters are the
fp16 outlier slices (`oweight`) of its QuantLinears.

The reference's finetune.py freezes every parameter except `*oweight*` and trains them through HF's LlamaForCausalLM loss
(cutoff_len 2048, labels of -100, gradient checkpointing).  Here:

    params = begin(model)                       every QuantLinear in training mode; the fp32 oweight parameters
    loss = causal_lm_loss(model, tokens, labels)
    loss.backward()                             dX / d(oweight) kernels per linear, qeft_lm_head_nll_grad at the head
    opt.step()                                  optim.OWeightAdamW(params): unscale, overflow check, global-norm clip, AdamW
    end(model)                                  back to inference: prefill, score and a new DecodeEngine see the trained weights

causal_lm_loss is a differentiable pass of its own (llama._prefill_pass, the inference route, is not touched): the linears and
the head run the project's kernels; norms, rotary, the activation and the residual adds are torch ops unless glue="fused" asks
for the project's row kernels and their backward kernels (qeft_amd.glue) and rope="fused" for the
project's rotary of q and k (glue.rope_qk), and so is attention unless attn="own" asks for the
project's own (attention.causal_attention).  The activations are fp16, so the loss is scaled against underflow -- opt.scale_loss(loss).backward(), the scale a device scalar
of the optimiser's that its update divides out again (or by hand: `(loss * s).backward()`, then divide the fp32 gradients by s);
the head's backward takes the scale in fp32 and keeps its softmax - onehot unscaled, so no scale makes it overflow or underflow there.
Sequences of unequal length go in as ONE packed row stream: pack_sequences(seqs) makes (tokens [R], labels, seq_lens) packs and
causal_lm_loss(model, tokens, labels, seq_lens=seq_lens) runs them -- the row-wise kernels over the R rows as they lie, the rotary
restarting per sequence, attention.causal_attention_packed keeping every sequence to itself.
train_step(model, opt, batches) is one whole update over a list of packed micro-batches: zero_grad, one scaled backward per
micro-batch, opt.step() (qeft_amd.optim.OWeightAdamW, DESIGN.md section 4.19: two launches, no host synchronisation);
warmup_constant_lr is the reference's schedule.  Trainer plumbing and datasets are out of scope.
"""
import math

import torch
from torch.utils.checkpoint import checkpoint as _checkpoint

from . import attention, glue as _glue, scoring
from .llama import layer_linears

IGNORE_INDEX = scoring.IGNORE_INDEX


def _linears(model):
    for L in model.model.layers:
        for _, ql in layer_linears(L):
            yield ql


def begin(model):
    """Put every QuantLinear into training mode (set_for_wct(), set_kernel(training=True)) and return the trainable parameters:
    the oweight slices, fp32 with requires_grad.  Everything else stays frozen."""
    params = []
    for ql in _linears(model):
        ql.set_for_wct()
        ql.set_kernel(training=True)
        if ql.outlierfeatures > 0:
            params.append(ql.oweight)
    return params


def end(model):
    """Back to inference after training: the interleaved copies the decode GEMV reads are re-derived, the prefill operands are
    dropped (rebuilt on the next prompt) and the model's oweight version is bumped as checkpoint.replace_oweight does, so a
    DecodeEngine built before refuses to run and a new one streams the trained weights."""
    for ql in _linears(model):
        ql.refresh_interleaved()
        ql.set_kernel(False)
    model._prefill_ops = None
    model._oweight_version = getattr(model, "_oweight_version", 0) + 1


def _check_seq_lens(tokens, seq_lens, max_seq=None):
    """seq_lens of a packed [R] token stream as a tuple of ints, or ValueError: 1-D tokens, 1 .. attention.MAX_SEQ lengths, each
    >= 1 (and <= max_seq where given), summing to R.  Looks at shapes alone: no launch, no device."""
    if tokens.dim() != 1:
        raise ValueError(f"seq_lens goes with 1-D packed tokens [R], got tokens {tuple(tokens.shape)}")
    lens = tuple(seq_lens)
    attention.seq_prefix(lens, tokens.shape[0])
    if max_seq is not None and max(lens) > max_seq:
        raise ValueError(f"a sequence of {max(lens)} tokens exceeds the model's max_seq {max_seq}")
    return lens


def shift_labels(tokens, labels=None, seq_lens=None):
    """HF's rule for a causal LM: row i is scored against labels[i + 1], the last row of every sequence is ignored.  tokens /
    labels [T] or [B, T]; labels default to the tokens.  seq_lens: tokens is a packed [R] stream of sequences of these lengths
    (pack_sequences), and the last row of EVERY packed sequence is ignored -- it has no successor of its own.  Returns int32 of
    the same shape."""
    labels = tokens if labels is None else labels
    if labels.shape != tokens.shape:
        raise ValueError(f"labels {tuple(labels.shape)} for tokens {tuple(tokens.shape)}")
    lens = None if seq_lens is None else _check_seq_lens(tokens, seq_lens)
    out = torch.full(labels.shape, IGNORE_INDEX, dtype=torch.int32, device=labels.device)
    out[..., :-1] = labels[..., 1:].to(torch.int32)
    if lens is not None:
        ends = torch.tensor(lens, dtype=torch.long).cumsum(0) - 1
        out[ends.to(out.device)] = IGNORE_INDEX
    return out


def pack_sequences(seqs, labels=None, budget=2048):
    """First-fit-decreasing packing of 1-D token tensors into row streams of at most `budget` rows and at most attention.MAX_SEQ
    sequences each -- what causal_lm_loss(seq_lens=...) takes.  Returns a list of (tokens [R], labels [R] or None, seq_lens);
    labels, where given, is a list of tensors shaped like `seqs`.  Sequences are placed longest first (ties in input order), each
    into the first pack with room, and stand in their pack in the order they were placed: deterministic, nothing dropped,
    nothing split.  CPU-side bookkeeping, no launch.  A sequence that is empty, not 1-D or longer than `budget` raises."""
    seqs = list(seqs)
    if labels is not None:
        labels = list(labels)
        if len(labels) != len(seqs) or any(l.shape != t.shape for l, t in zip(labels, seqs)):
            raise ValueError("labels must be a list of tensors shaped like seqs")
    for i, t in enumerate(seqs):
        if t.dim() != 1 or t.shape[0] < 1:
            raise ValueError(f"sequence {i} must be 1-D with at least one token, got {tuple(t.shape)}")
        if t.shape[0] > budget:
            raise ValueError(f"sequence {i} has {t.shape[0]} tokens, more than the budget of {budget} rows")
    packs = []                                                          # [rows, [indices]]
    for i in sorted(range(len(seqs)), key=lambda j: -seqs[j].shape[0]):           # stable: ties stay in input order
        n = seqs[i].shape[0]
        for pk in packs:
            if pk[0] + n <= budget and len(pk[1]) < attention.MAX_SEQ:
                pk[0] += n
                pk[1].append(i)
                break
        else:
            packs.append([n, [i]])
    return [(torch.cat([seqs[i] for i in idx]), None if labels is None else torch.cat([labels[i] for i in idx]),
             [int(seqs[i].shape[0]) for i in idx]) for _, idx in packs]


def _rmsnorm(x, gamma, eps):
    xf = x.float()
    return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * gamma.float()).half()


def _rope(x, cos, sin):
    """x [B, T, H, 128] fp16, cos / sin [T, 1, 64] fp32 -> rotated fp16 (fp32 math), the pairing of llama._prefill_pass."""
    a, b = x[..., :64].float(), x[..., 64:].float()
    return torch.cat([a * cos - b * sin, b * cos + a * sin], dim=-1).half()


def _attend(q, k, v, s, B, T, own_attn, seq_lens=None):
    """q [B, T, H, 128], k / v [B, T, Hkv, 128] (rotated) -> [B * T, hidden] on either attention route.  seq_lens: B = 1 and the T
    rows are packed sequences of these lengths -- one causal_attention_packed call, or SDPA once per sequence (the comparison
    route, not a fast one)."""
    if own_attn:
        if seq_lens is not None:
            return attention.causal_attention_packed(q[0], k[0], v[0], seq_lens).reshape(T, s.hidden)
        return attention.causal_attention(q, k, v).reshape(B * T, s.hidden)
    rep = s.n_heads // s.n_kv_heads
    if rep != 1:
        k, v = k.repeat_interleave(rep, 2), v.repeat_interleave(rep, 2)
    if seq_lens is not None:
        parts, a = [], 0
        for n in seq_lens:
            parts.append(torch.nn.functional.scaled_dot_product_attention(
                q[:, a:a + n].transpose(1, 2), k[:, a:a + n].transpose(1, 2), v[:, a:a + n].transpose(1, 2), is_causal=True))
            a += n
        return torch.cat(parts, dim=2).transpose(1, 2).reshape(T, s.hidden)
    a = torch.nn.functional.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), is_causal=True)
    return a.transpose(1, 2).reshape(B * T, s.hidden)


def _rope_qk(q, k, cos, sin, fused):
    """q and k rotated: the torch expression twice, or one glue.rope_qk launch with the same bits (cos / sin [T, 1, 64])."""
    if fused:
        return _glue.rope_qk(q, k, cos[:, 0], sin[:, 0])
    return _rope(q, cos, sin), _rope(k, cos, sin)


def _decoder_layer(h, L, s, B, T, cos, sin, own_attn=False, fused_rope=False, seq_lens=None):
    """h [B * T, hidden] fp16 -> the layer's output, fp16; every linear is the module's own forward (training mode: the MFMA
    forward, dX and d(oweight) kernels; o_proj gathers its own column order).  own_attn: attention.causal_attention on the
    un-repeated k / v instead of torch's SDPA; fused_rope: glue.rope_qk instead of the two _rope expressions."""
    at, mlp = L.self_attn, L.mlp
    x = _rmsnorm(h, L.input_layernorm.weight, s.rms_eps)
    q, k = _rope_qk(at.q_proj(x).view(B, T, s.n_heads, 128), at.k_proj(x).view(B, T, s.n_kv_heads, 128), cos, sin, fused_rope)
    v = at.v_proj(x).view(B, T, s.n_kv_heads, 128)
    h = h + at.o_proj(_attend(q, k, v, s, B, T, own_attn, seq_lens))
    x = _rmsnorm(h, L.post_attention_layernorm.weight, s.rms_eps)
    act = (torch.nn.functional.silu(mlp.gate_proj(x).float()) * mlp.up_proj(x).float()).half()
    return h + mlp.down_proj(act)


def _decoder_layer_fused(h, delta, L, s, B, T, cos, sin, own_attn=False, fused_rope=False, seq_lens=None):
    """The layer of glue="fused" (DESIGN.md section 4.16).  The residual stream arrives as (h, delta) -- the stream before the last
    MLP and that MLP's output, delta None in layer 0 -- and leaves the same way, so that every residual add happens inside the
    norm that follows it (glue.add_rmsnorm) and every sum of residual-stream gradients inside that norm's backward; SiLU * up is
    glue.swiglu.  The rotary is the torch expression of the default route unless fused_rope asks for glue.rope_qk."""
    at, mlp = L.self_attn, L.mlp
    s1, x = _glue.add_rmsnorm(h, delta, L.input_layernorm.weight, s.rms_eps)
    q, k = _rope_qk(at.q_proj(x).view(B, T, s.n_heads, 128), at.k_proj(x).view(B, T, s.n_kv_heads, 128), cos, sin, fused_rope)
    v = at.v_proj(x).view(B, T, s.n_kv_heads, 128)
    s2, x = _glue.add_rmsnorm(s1, at.o_proj(_attend(q, k, v, s, B, T, own_attn, seq_lens)), L.post_attention_layernorm.weight, s.rms_eps)
    act = _glue.swiglu(mlp.gate_proj(x), mlp.up_proj(x))
    return s2, mlp.down_proj(act)


def causal_lm_loss(model, tokens, labels=None, *, seq_lens=None, checkpoint=True, head="fused", attn="sdpa", glue="torch",
                   rope="torch"):
    """Mean NLL (fp32 scalar) of the shifted labels under `model`, differentiable with respect to the oweight parameters that
    begin(model) returned.  tokens [T] or [B, T] (right-padded; label the padding -100), labels as shift_labels takes them; a
    label outside [0, vocab) is ignored, and the mean runs over the others (0 when there is none).  Every sequence starts at
    position 0.  seq_lens (Python ints): tokens is ONE packed stream [R] of sequences of these lengths (pack_sequences makes
    them) -- every row-wise kernel runs over the R rows as they lie, the rotary restarts at 0 for every
    sequence, each sequence attends itself alone (attn="own": one attention.causal_attention_packed call; attn="sdpa": SDPA
    once per sequence) and the last row of every sequence is ignored.  ValueError, before any launch, for 2-D tokens, lengths
    that do not sum to R, a length below 1 or above max_seq, or more than attention.MAX_SEQ sequences.  checkpoint=True recomputes each decoder layer in the backward (torch.utils.checkpoint, use_reentrant=False), as
    the reference's gradient checkpointing does.  head="fused": scoring.lm_head_nll_loss, no [T, vocab] tensor in either
    direction; head="torch": hn @ W.t() -> fp32 -> cross_entropy, the route the fused head is measured against.
    attn="sdpa": torch's scaled_dot_product_attention over k / v repeated to the query heads; attn="own":
    attention.causal_attention, the project's forward and backward kernels on the un-repeated k / v.
    glue="torch": norms, rotary, SiLU * up and the residual adds are torch ops; glue="fused": norms and SiLU * up on the project's
    row kernels and their backward kernels (qeft_amd.glue), with every residual add inside the norm that
    follows it.  rope="torch": the rotary of q and k is finetune._rope, twice per layer, on either glue; rope="fused":
    one glue.rope_qk launch per layer and one for its backward, the same bits in both directions, with
    either glue and either attn.
    fp16 activations: scale the loss, opt.scale_loss(loss).backward() (optim.OWeightAdamW) or `(loss * s).backward()` by hand."""
    if head not in ("fused", "torch"):
        raise ValueError(f"head must be 'fused' or 'torch', got {head!r}")
    if attn not in ("sdpa", "own"):
        raise ValueError(f"attn must be 'sdpa' or 'own', got {attn!r}")
    if glue not in ("torch", "fused"):
        raise ValueError(f"glue must be 'torch' or 'fused', got {glue!r}")
    if rope not in ("torch", "fused"):
        raise ValueError(f"rope must be 'torch' or 'fused', got {rope!r}")
    s = model.shape
    own, frope = attn == "own", rope == "fused"
    if own and (s.n_heads % s.n_kv_heads != 0 or s.hidden != s.n_heads * 128):
        raise ValueError(f"attn='own' takes heads of 128 and n_heads % n_kv_heads == 0, got hidden {s.hidden}, "
                         f"{s.n_heads} / {s.n_kv_heads} heads")
    lens = None if seq_lens is None else _check_seq_lens(tokens, seq_lens, s.max_seq)
    dev = model.lm_head.weight.device
    tokens = tokens.to(dev)
    if tokens.dim() not in (1, 2):
        raise ValueError(f"tokens must be [T] or [B, T], got {tuple(tokens.shape)}")
    targets = shift_labels(tokens, None if labels is None else labels.to(dev), lens).reshape(-1)
    tok2 = tokens.reshape(-1, tokens.shape[-1])
    B, T = tok2.shape
    if lens is None:
        if T > s.max_seq:
            raise ValueError(f"{T} tokens exceed the model's max_seq {s.max_seq}")
        cos, sin = model.rope_cos[:T, None, :], model.rope_sin[:T, None, :]
    else:                                                               # B = 1, T = R; positions restart with every sequence
        pos = torch.cat([torch.arange(n) for n in lens]).to(dev)
        cos, sin = model.rope_cos[pos][:, None, :], model.rope_sin[pos][:, None, :]
    h = model.model.embed_tokens.weight[tok2.reshape(-1)]              # [B * T, hidden] fp16
    if glue == "fused":
        delta = None
        for L in model.model.layers:
            if checkpoint:
                h, delta = _checkpoint(_decoder_layer_fused, h, delta, L, s, B, T, cos, sin, own, frope, lens, use_reentrant=False)
            else:
                h, delta = _decoder_layer_fused(h, delta, L, s, B, T, cos, sin, own, frope, lens)
        hn = _glue.add_rmsnorm(h, delta, model.model.norm.weight, s.rms_eps)[1]
    else:
        for L in model.model.layers:
            if checkpoint:
                h = _checkpoint(_decoder_layer, h, L, s, B, T, cos, sin, own, frope, lens, use_reentrant=False)
            else:
                h = _decoder_layer(h, L, s, B, T, cos, sin, own, frope, lens)
        hn = _rmsnorm(h, model.model.norm.weight, s.rms_eps)
    W = model.lm_head.weight
    ok = (targets >= 0) & (targets < s.vocab)
    n = ok.sum().clamp_min(1).to(torch.float32)
    if head == "fused":
        return scoring.lm_head_nll_loss(hn, W, targets).sum() / n
    logits = torch.matmul(hn, W.t()).float()
    lab = torch.where(ok, targets, torch.full_like(targets, IGNORE_INDEX)).long()
    return torch.nn.functional.cross_entropy(logits, lab, ignore_index=IGNORE_INDEX, reduction="sum") / n


def warmup_constant_lr(i, total, base, warmup_ratio=0.03):
    """The reference's schedule (a constant learning rate behind a linear warm-up over warmup_ratio of the run) as a pure function:
    the rate of update i (0-based) of `total`.  The warm-up lasts ceil(total * warmup_ratio) updates and update i of it runs at
    base * i / that count -- the first at 0, as the scheduler the reference's Trainer builds does; from there on `base`."""
    if total < 1 or i < 0:
        raise ValueError(f"update {i} of {total}")
    warmup = math.ceil(total * warmup_ratio)
    return base * i / max(1.0, warmup) if i < warmup else base


def train_step(model, opt, batches, **loss_kwargs):
    """One update of the oweight parameters: opt.zero_grad(); for every (tokens, labels, seq_lens) of `batches` (what
    pack_sequences returns; labels and seq_lens may be None) the backward of opt.scale_loss(causal_lm_loss(...), accum=len(batches));
    opt.step().  loss_kwargs go to causal_lm_loss (attn, glue, rope, head, checkpoint).  Returns the unscaled mean of the
    micro-batch losses as a device scalar; nothing here synchronises the host.  A step whose gradient overflowed is skipped by the
    optimiser (opt.stats() tells), the returned loss is that of the forward passes either way."""
    batches = list(batches)
    if not batches:
        raise ValueError("train_step needs at least one micro-batch")
    opt.zero_grad()
    total = None
    for tokens, labels, seq_lens in batches:
        loss = causal_lm_loss(model, tokens, labels, seq_lens=seq_lens, **loss_kwargs)
        opt.scale_loss(loss, accum=len(batches)).backward()
        total = loss.detach() if total is None else total + loss.detach()
    opt.step()
    return total / len(batches)
