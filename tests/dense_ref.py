"""One dense reference for whole passes of a QuantLlama (the GPU tests' yardstick).

dense_pass() is a causal forward over `model.dense_weights()` (a 3-bit layer arrives there expanded through _qweight4), written
with plain torch ops, in one of two modes:

  F64   everything in fp64: the reference.
  F16   fp16 tensors and plain torch ops, rounded where the project's passes round (norm, rotary and activation in fp32 then fp16;
        fp16 matmuls and attention; an fp16 residual stream; an fp16 lm_head matmul; fp32 cross-entropy of the fp16 logits).
        This is the fp16 torch pass the project's routes are measured against: a route may be off the fp64 pass by at most twice
        what this pass is, plus a floor of the output format (bounded() below).

It returns either the logits [B * T, vocab] (fp64 / fp16) or the mean NLL of `targets`.  With `leaves` each linear's last n_out
columns come from leaves[li][name], so autograd reaches the outlier slices (tests/test_gpu_lm_head_nll_grad.py)."""
import math

import torch

F16, F32, F64 = torch.float16, torch.float32, torch.float64
IGNORE = -100


def dense_pass(model, dense, leaves, tok2, targets, dt, out="nll"):
    """Causal pass of tok2 [B, T] (every sequence from position 0) over dense weights; each linear's last n_out columns are
    leaves[li][name] where `leaves` is given.  dt = F64 or F16 (module docstring).  out = "nll": the mean NLL of targets [B * T]
    (IGNORE rows left out); out = "logits": the logits [B * T, vocab] in dt (targets is not read)."""
    s = model.shape
    lo = dt == F16
    up = F32 if lo else F64
    B, T = tok2.shape
    cos, sin = model.rope_cos[:T, None, :].to(up), model.rope_sin[:T, None, :].to(up)
    rep = s.n_heads // s.n_kv_heads

    def rms(x, g):
        xf = x.to(up)
        return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + s.rms_eps) * g.to(up)).to(dt)

    def rope(x):
        a, b = x[..., :64].to(up), x[..., 64:].to(up)
        return torch.cat([a * cos - b * sin, b * cos + a * sin], dim=-1).to(dt)

    def lin(x, li, name):
        W = dense[li][name].to(dt)
        if leaves is not None:
            leaf = leaves[li][name]
            W = torch.cat([W[:, :-leaf.shape[1]], leaf.to(dt)], dim=1)
        return x @ W.t()

    h = model.model.embed_tokens.weight[tok2.reshape(-1)].to(dt)
    for li, L in enumerate(model.model.layers):
        x = rms(h, L.input_layernorm.weight)
        q = rope(lin(x, li, "q_proj").view(B, T, s.n_heads, 128))
        k = rope(lin(x, li, "k_proj").view(B, T, s.n_kv_heads, 128))
        v = lin(x, li, "v_proj").view(B, T, s.n_kv_heads, 128)
        if rep != 1:
            k, v = k.repeat_interleave(rep, 2), v.repeat_interleave(rep, 2)
        a = torch.nn.functional.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), is_causal=True)
        a = a.transpose(1, 2).reshape(B * T, s.hidden)
        if hasattr(L.self_attn.o_proj, "reorder_ids"):
            a = a[:, L.self_attn.o_proj.reorder_ids]
        h = h + lin(a, li, "o_proj")
        x = rms(h, L.post_attention_layernorm.weight)
        act = (torch.nn.functional.silu(lin(x, li, "gate_proj").to(up)) * lin(x, li, "up_proj").to(up)).to(dt)
        h = h + lin(act, li, "down_proj")
    hn = rms(h, model.model.norm.weight)
    logits = hn @ model.lm_head.weight.to(dt).t()
    if out == "logits":
        return logits
    assert out == "nll", out
    return torch.nn.functional.cross_entropy(logits.to(up), targets.long(), ignore_index=IGNORE, reduction="mean")


@torch.no_grad()
def logits_pair(model, tokens, dense=None):
    """(ref64, logits16) of tokens [T]: the fp64 logits [T, vocab] and the fp16 torch pass's (as fp64), no gradients."""
    dense = dense if dense is not None else model.dense_weights()
    tok2 = tokens.reshape(1, -1).to(model.lm_head.weight.device)
    ref64 = dense_pass(model, dense, None, tok2, None, F64, out="logits")
    l16 = dense_pass(model, dense, None, tok2, None, F16, out="logits")
    return ref64, l16.to(F64)


def next_token_nll(logits, tokens):
    """Mean NLL of tokens[1:] under logits[:-1] (llama.nll_from_logits' protocol): fp64 logits in fp64, any others in fp32 as
    the project's passes take theirs."""
    lg = logits[:-1] if logits.dtype == F64 else logits[:-1].float()
    return torch.nn.functional.cross_entropy(lg, tokens[1:].to(logits.device).long()).item()


def ulp16(v):
    """One fp16 ulp at |v| (2^-24 below the normal range)."""
    return 2.0 ** (math.floor(math.log2(max(abs(v), 2.0 ** -14))) - 10)


def max_err(a, ref64):
    return (a.to(F64) - ref64).abs().max().item()


def bounded(tag, e_own, e_16, floor, what="logits"):
    """The project's rule for a route measured against the fp16 torch pass (test_causal_lm_loss_on_the_tiny_model): own error from
    fp64 <= 2 x the fp16 torch pass's + a floor of the output format.  Prints the figures, then asserts."""
    print(f"[dense_ref] {tag}: {what} |d| own {e_own:.4e}  fp16 torch {e_16:.4e}  ratio {e_own / max(e_16, 1e-300):.3f} "
          f"(allowed 2 x + {floor:.3e})")
    assert e_own <= 2 * e_16 + floor, f"{tag}: {what} error {e_own:.4e} > 2 x {e_16:.4e} + {floor:.3e}"
    return e_own / max(e_16, 1e-300)


NLL_FLOOR = 2.0 ** -14          # the loss floor of test_causal_lm_loss_on_the_tiny_model


def check_logits_and_nll(tag, got, ref64, l16, tokens, rows=slice(None)):
    """got [T', vocab] (the rows `rows` of a teacher-forced pass over `tokens`) against the fp64 pass, both bounded by the fp16
    torch pass: the largest logit error (floor: one fp16 ulp of the largest reference logit) and, over whole passes, the next-token
    NLL (floor 2^-14).  Returns (e_own, e_16)."""
    ref, f16 = ref64[rows], l16[rows]
    assert torch.isfinite(got).all(), f"{tag}: non-finite logits"
    e_own, e_16 = max_err(got, ref), max_err(f16, ref)
    bounded(tag, e_own, e_16, ulp16(ref.abs().max().item()))
    if got.shape[0] == tokens.numel():
        n64 = next_token_nll(ref64, tokens)
        bounded(tag, abs(next_token_nll(got, tokens) - n64), abs(next_token_nll(l16.half(), tokens) - n64), NLL_FLOOR, "nll")
    return e_own, e_16
