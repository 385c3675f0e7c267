"""Scoring on the project's own path: log-probabilities, perplexity.

The reference's headline quality number is perplexity: qeft/main.py:196-308 (eval_ppl) runs 2048-token windows through the
model and takes CrossEntropyLoss on shifted labels; its fine-tune loop is the same loss with -100 labels.  Here the prompt pass
(llama.prefill's, caches and chunking included) stops at the final-norm rows and qeft_lm_head_nll turns them into per-row
log-sum-exp, target logit and argmax: fp32 logits that never pass through fp16, and no [T, vocab] tensor.

    score(model, tokens)        per-token log-probabilities of a document (optionally on an engine's cache, in chunks)
    eval_nll(model, tokens)     the reference's perplexity protocol over windows of `seqlen` tokens
    lm_head_nll(hn, weight)     the kernel's thin wrapper
    lm_head_nll_loss(hn, weight, targets)   the same head as a differentiable per-row NLL (section 4.14): the backward is
                                qeft_lm_head_nll_grad, again without a [T, vocab] tensor; finetune.causal_lm_loss ends in it
"""
import math
from dataclasses import dataclass

import torch

from . import _lib, llama

IGNORE_INDEX = -100          # the reference's label for "no loss here" (any target outside [0, vocab) is ignored)
_QEFT_ERR_SHAPE = 2

_workspace = {}              # device -> uint8 buffer, grown on demand; one stream at a time uses it (as the engines' buffers)
_grad_workspace = {}         # the same for qeft_lm_head_nll_grad: at most chunk_rows rows of g, whatever T


@dataclass
class Score:
    """score()'s result, one entry per token row."""
    logprob: torch.Tensor    # fp32 [T]: log p(target | prefix) = tgt_logit - lse; 0 on ignored rows
    lse: torch.Tensor        # fp32 [T]: log sum exp of the row's logits
    argmax: torch.Tensor     # int32 [T]: the greedy token, lowest index among equal maxima


def _lm_head_nll_torch(hn, weight, targets):
    """The same three tensors with torch on the GPU in fp32, for a width the kernel does not take (as DecodeEngine._head's torch
    route for odd widths).  It does build the [T, vocab] logits."""
    logits = hn.float() @ weight.float().t()
    vocab = logits.shape[1]
    mx = logits.max(dim=1, keepdim=True).values
    lse = torch.logsumexp(logits, dim=1)
    idx = torch.arange(vocab, device=logits.device, dtype=torch.int32).expand_as(logits)
    argmax = torch.where(logits == mx, idx, torch.full_like(idx, vocab)).min(dim=1).values.to(torch.int32)
    tgt = None
    if targets is not None:
        ok = (targets >= 0) & (targets < vocab)
        got = logits.gather(1, targets.clamp(0, vocab - 1).long()[:, None])[:, 0]
        tgt = torch.where(ok, got, torch.zeros_like(got))
    return lse, tgt, argmax


@torch.no_grad()
def lm_head_nll(hn, weight, targets=None):
    """hn fp16 [T, hidden] (final-norm rows; a row-strided view is taken as it lies), weight fp16 [vocab, hidden], targets
    integer [T] or None -> (lse fp32 [T], tgt_logit fp32 [T] or None, argmax int32 [T]) through qeft_lm_head_nll
    (include/qeft_hip.h): logits accumulated in fp32, never rounded to fp16, never stored.  A target outside [0, vocab) is
    ignored: its tgt_logit is 0.  A shape the entry refuses (hidden % 64 != 0) is computed by torch in fp32 on the GPU."""
    if not (hn.is_cuda and weight.is_cuda):
        raise RuntimeError("lm_head_nll needs GPU tensors (there is no CPU path)")
    if hn.dtype != torch.float16 or weight.dtype != torch.float16 or hn.dim() != 2 or weight.dim() != 2 \
            or hn.shape[1] != weight.shape[1]:
        raise ValueError(f"lm_head_nll takes fp16 hn [T, hidden] and weight [vocab, hidden], got {tuple(hn.shape)} {hn.dtype}, "
                         f"{tuple(weight.shape)} {weight.dtype}")
    T, hidden = hn.shape
    vocab = weight.shape[0]
    dev = hn.device
    if targets is not None:
        if targets.numel() != T:
            raise ValueError(f"{targets.numel()} targets for {T} rows")
        targets = targets.to(device=dev, dtype=torch.int32).contiguous()
    lib = _lib.lib()
    need = lib.qeft_lm_head_nll_workspace_bytes(T, vocab)
    if T == 0 or need == 0 or hidden % 64 != 0:
        return _lm_head_nll_torch(hn, weight, targets)
    if hn.stride(1) != 1 or hn.stride(0) % 8 != 0 or hn.stride(0) < hidden or hn.data_ptr() % 16 != 0:
        hn = hn.contiguous()
    weight = weight.contiguous()
    ws = _workspace.get(dev)
    if ws is None or ws.numel() < need:
        _workspace[dev] = None
        ws = _workspace[dev] = torch.empty(need, dtype=torch.uint8, device=dev)
    lse = torch.empty(T, dtype=torch.float32, device=dev)
    argmax = torch.empty(T, dtype=torch.int32, device=dev)
    tgt = torch.empty(T, dtype=torch.float32, device=dev) if targets is not None else None
    code = lib.qeft_lm_head_nll(hn.data_ptr(), hn.stride(0), weight.data_ptr(), targets.data_ptr() if targets is not None else None,
                                lse.data_ptr(), tgt.data_ptr() if tgt is not None else None, argmax.data_ptr(), ws.data_ptr(),
                                ws.numel(), T, hidden, vocab, torch.cuda.current_stream(dev).cuda_stream)
    if code == _QEFT_ERR_SHAPE:
        return _lm_head_nll_torch(hn, weight, targets)
    _lib.check(code)
    return lse, tgt, argmax


def _nll_torch(hn, weight, targets):
    """nll [T] in fp32 by differentiable torch ops, for a width the entries do not take.  It does build the [T, vocab] logits."""
    logits = hn.float() @ weight.float().t()
    vocab = logits.shape[1]
    ok = (targets >= 0) & (targets < vocab)
    got = logits.gather(1, targets.clamp(0, vocab - 1).long()[:, None])[:, 0]
    nll = torch.logsumexp(logits, dim=1) - got
    return torch.where(ok, nll, torch.zeros_like(nll))


def _entry_view(hn, hidden):
    """hn as the entries take it: unit column stride, rows a multiple of 8 elements apart, 16-byte aligned."""
    if hn.stride(1) != 1 or hn.stride(0) % 8 != 0 or hn.stride(0) < hidden or hn.data_ptr() % 16 != 0:
        hn = hn.contiguous()
    return hn


@torch.no_grad()
def lm_head_nll_grad(hn, weight, targets, lse, grad_nll, fp32=False):
    """d(sum_i grad_nll_i nll_i) / d hn through qeft_lm_head_nll_grad (include/qeft_hip.h): hn, weight, targets as lm_head_nll's,
    lse its first result, grad_nll fp32 [T] -> fp16 [T, hidden] (fp32 with fp32=True); rows with an ignored target are +0.0.
    The workspace is cached per device and holds at most chunk_rows rows of g."""
    T, hidden = hn.shape
    vocab = weight.shape[0]
    dev = hn.device
    lib = _lib.lib()
    need = lib.qeft_lm_head_nll_grad_workspace_bytes(T, hidden, vocab)
    if need == 0:
        raise ValueError(f"qeft_lm_head_nll_grad does not take T={T}, hidden={hidden}, vocab={vocab}")
    hn = _entry_view(hn, hidden)
    weight = weight.contiguous()
    targets = targets.to(device=dev, dtype=torch.int32).contiguous()
    lse = lse.to(device=dev, dtype=torch.float32).contiguous()
    grad_nll = grad_nll.to(device=dev, dtype=torch.float32).contiguous()
    ws = _grad_workspace.get(dev)
    if ws is None or ws.numel() < need:
        _grad_workspace[dev] = None
        ws = _grad_workspace[dev] = torch.empty(need, dtype=torch.uint8, device=dev)
    dx = torch.empty(T, hidden, dtype=torch.float32 if fp32 else torch.float16, device=dev)
    _lib.check(lib.qeft_lm_head_nll_grad(hn.data_ptr(), hn.stride(0), weight.data_ptr(), targets.data_ptr(), lse.data_ptr(),
                                         grad_nll.data_ptr(), dx.data_ptr(), hidden, int(fp32), ws.data_ptr(), ws.numel(), T, hidden,
                                         vocab, torch.cuda.current_stream(dev).cuda_stream))
    return dx


class _LmHeadNllLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hn, weight, targets):
        # rows are independent bit for bit (section 4.13), so the forward runs in pieces of the backward's chunk: neither
        # workspace grows with T
        R = _lib.lib().qeft_lm_head_nll_grad_chunk_rows(hn.shape[1], weight.shape[0])
        parts = [lm_head_nll(hn[a:a + R], weight, targets[a:a + R])[:2] for a in range(0, hn.shape[0], R)]
        lse = parts[0][0] if len(parts) == 1 else torch.cat([p[0] for p in parts])
        tgt = parts[0][1] if len(parts) == 1 else torch.cat([p[1] for p in parts])
        ok = (targets >= 0) & (targets < weight.shape[0])
        ctx.save_for_backward(hn, weight, lse, targets)
        return torch.where(ok, lse - tgt, torch.zeros_like(lse))

    @staticmethod
    def backward(ctx, grad_nll):
        hn, weight, lse, targets = ctx.saved_tensors
        return lm_head_nll_grad(hn, weight, targets, lse, grad_nll), None, None


def lm_head_nll_loss(hn, weight, targets):
    """nll fp32 [T] = lse - tgt_logit of lm_head_nll (bit for bit; 0 on rows whose target is outside [0, vocab)), differentiable
    with respect to hn: the backward is qeft_lm_head_nll_grad and returns fp16 [T, hidden].  Neither direction builds a
    [T, vocab] tensor in torch; the backward's workspace holds at most 1024 rows of fp16 (softmax - onehot).  The lm_head is
    frozen in QEFT: a weight that requires grad raises.  A width the entries refuse (hidden % 64 != 0) takes a differentiable
    torch fp32 route, as lm_head_nll's forward does."""
    if weight.requires_grad:
        raise ValueError("lm_head_nll_loss has no gradient for the weight: QEFT never trains the lm_head (freeze it)")
    if not (hn.is_cuda and weight.is_cuda):
        raise RuntimeError("lm_head_nll_loss needs GPU tensors (there is no CPU path)")
    if hn.dtype != torch.float16 or weight.dtype != torch.float16 or hn.dim() != 2 or weight.dim() != 2 \
            or hn.shape[1] != weight.shape[1]:
        raise ValueError(f"lm_head_nll_loss takes fp16 hn [T, hidden] and weight [vocab, hidden], got {tuple(hn.shape)} {hn.dtype}, "
                         f"{tuple(weight.shape)} {weight.dtype}")
    T, hidden = hn.shape
    if targets.numel() != T:
        raise ValueError(f"{targets.numel()} targets for {T} rows")
    targets = targets.to(device=hn.device, dtype=torch.int32).reshape(T).contiguous()
    if T == 0 or _lib.lib().qeft_lm_head_nll_grad_workspace_bytes(T, hidden, weight.shape[0]) == 0:
        return _nll_torch(hn, weight, targets)
    return _LmHeadNllLoss.apply(hn, weight, targets)


@torch.no_grad()
def score(model, tokens, engine=None, *, start=0, attn=None, chunk=None, targets=None):
    """Per-token log-probabilities of `tokens` [T] under `model`: the prompt pass of llama.prefill -- engine, start, attn and chunk
    mean exactly what they mean there; the caches are filled and the position is set -- ending in qeft_lm_head_nll instead of the
    lm_head matmul.  targets [T]: row i is scored against targets[i]; the default is the next token, tokens[1:] followed by one
    ignored entry.  A target outside [0, vocab) (IGNORE_INDEX = -100 among them) is ignored: logprob 0 there.  Single GPU, as
    prefill.  Returns a Score(logprob, lse, argmax); no [T, vocab] tensor is allocated."""
    dev = model.lm_head.weight.device
    tokens = tokens.to(dev)
    T = tokens.numel()
    if targets is None:
        targets = torch.cat([tokens[1:].to(torch.int32), torch.full((1,), IGNORE_INDEX, dtype=torch.int32, device=dev)])
    elif targets.numel() != T:
        raise ValueError(f"{targets.numel()} targets for {T} tokens")
    targets = targets.to(device=dev, dtype=torch.int32)
    hn = llama.prefill(model, tokens, engine, start=start, attn=attn, chunk=chunk, _head=False)
    lse, tgt, argmax = lm_head_nll(hn, model.lm_head.weight, targets)
    ok = (targets >= 0) & (targets < model.shape.vocab)
    return Score(torch.where(ok, tgt - lse, torch.zeros_like(lse)), lse, argmax)


@torch.no_grad()
def eval_nll(model, tokens, seqlen=2048, chunk=None):
    """The reference's perplexity protocol (qeft/main.py:196-305): n = tokens.numel() // seqlen windows, each run from position 0
    (a trailing partial window is dropped); per window the mean NLL over its seqlen - 1 shifted targets, times seqlen;
    nll = sum of the windows / (n * seqlen), ppl = exp(nll).  The window sums are accumulated in fp64.  chunk: run each window in
    pieces of at most `chunk` tokens (score's chunk).  Returns {"nll", "ppl", "windows", "tokens"}."""
    seqlen = int(seqlen)
    if seqlen < 2:
        raise ValueError(f"seqlen must be >= 2 (a window has seqlen - 1 shifted targets), got {seqlen}")
    if seqlen > model.shape.max_seq:
        raise ValueError(f"seqlen {seqlen} exceeds the model's max_seq {model.shape.max_seq}")
    tokens = tokens.reshape(-1)
    n = tokens.numel() // seqlen
    if n == 0:
        raise ValueError(f"{tokens.numel()} tokens do not fill one window of {seqlen}")
    total = 0.0
    for i in range(n):
        sc = score(model, tokens[i * seqlen:(i + 1) * seqlen], chunk=chunk)
        mean = -float(sc.logprob[:seqlen - 1].double().sum().item()) / (seqlen - 1)
        total += mean * seqlen
    nll = total / (n * seqlen)
    return {"nll": nll, "ppl": math.exp(nll), "windows": n, "tokens": n * seqlen}
