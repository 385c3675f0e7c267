"""Assisted (speculative) decoding on the decode engine's verify pass (DecodeEngine.verify / verify_sample), greedy or sampled.

A draft proposes up to k next tokens; the target scores the last accepted token and the k drafts in ONE pass of m = k + 1 rows
(every weight byte streams once for all rows) and keeps the longest prefix of drafts that equal its own greedy choices, plus
its own next token.  The result is the target's plain greedy sequence (up to the rounding of m-row vs one-row launches), at
up to k + 1 tokens per pass.

Under sampling (assisted_generate(..., sampling=SamplingParams)) the target draws row i with its record at the position the
token will occupy, exactly as a sampled step() would, and keeps the drafts that equal these draws: the output is the token
stream of sampled run() with the same record, whatever the draft proposes.

Two drafts:
  EngineDraft        a second DecodeEngine with the same vocabulary (a shallower or 3-bit model); its KV cache is rolled back
                     with set_position() to the accepted prefix before it drafts again.  Greedy, or with set_sampling() drawing
                     its proposals with the target's record: the same uniform at every position (common random numbers);
  PromptLookupDraft  an n-gram match in the context (host only): for users without a draft model.
"""
import torch


def accepted_prefix(argmax_rows, tokens):
    """The acceptance rule of the verify pass in plain Python: n = the longest prefix with argmax_rows[i] == tokens[i + 1];
    returns (n, tokens[1..n] + [argmax_rows[n]]).  argmax_rows are the target's per-row choices, whatever made them: the
    argmax of row i (qeft_verify_greedy) or the draw of row i at its position (qeft_verify_sample)."""
    m = len(tokens)
    n = 0
    while n < m - 1 and int(argmax_rows[n]) == int(tokens[n + 1]):
        n += 1
    return n, [int(t) for t in tokens[1:n + 1]] + [int(argmax_rows[n])]


class PromptLookupDraft:
    """Drafts by looking the context's last n tokens up earlier in the context (longest n first, most recent match first)
    and proposing what followed there.  No model, no device work."""

    def __init__(self, max_ngram=3, min_ngram=1):
        assert 1 <= min_ngram <= max_ngram
        self.max_ngram, self.min_ngram = max_ngram, min_ngram

    def propose(self, context, k):
        if k <= 0:
            return []
        ctx = [int(t) for t in context]
        L = len(ctx)
        for n in range(min(self.max_ngram, L - 1), self.min_ngram - 1, -1):
            tail = ctx[L - n:]
            for start in range(L - n - 1, -1, -1):
                if ctx[start:start + n] == tail:
                    cand = ctx[start + n:start + n + k]
                    if cand:
                        return cand
        return []


class EngineDraft:
    """A second DecodeEngine as the draft model.  It keeps the tokens whose K/V its cache holds (positions 0 ..); before
    drafting it rolls back to the part of that history the context still agrees with (set_position), feeds what it has not
    seen, then decodes k tokens: greedily, or drawn with the record of set_sampling()."""

    def __init__(self, engine):
        self.eng = engine
        self.hist = []          # token at each position of the draft's KV cache
        self.sampling = None    # SamplingParams (seed resolved) the proposals are drawn with; None: greedy
        self.eng.reset()

    def set_sampling(self, params):
        """Draw the proposals with `params` (None: greedy again).  A step() of the draft draws at the position its token will
        occupy, so with the target's record the draft uses the very uniform the target will use there: where the two
        distributions are close, their inverse CDFs agree and the draft is accepted."""
        self.sampling = params.resolved() if params is not None else None

    def propose(self, context, k):
        eng = self.eng
        ctx = [int(t) for t in context]
        k = min(k, eng.m.shape.max_seq - len(ctx))
        if k <= 0:
            return []
        c = 0
        while c < min(len(self.hist), len(ctx) - 1) and self.hist[c] == ctx[c]:
            c += 1
        eng.set_position(c)
        del self.hist[c:]
        eng.set_sampling(None)
        eng.greedy = False
        for t in ctx[c:-1]:                     # the context the draft has not seen (teacher-forced)
            eng.tok.fill_(t)
            eng.step()
            self.hist.append(t)
        eng.greedy = True
        eng.set_sampling(self.sampling)
        out = []
        eng.tok.fill_(ctx[-1])
        self.hist.append(ctx[-1])
        for i in range(k):
            eng.step()                          # consumes tok, writes its successor (argmax or draw) into tok
            t = int(eng.tok.item())
            out.append(t)
            if i + 1 < k:
                self.hist.append(t)
        return out


@torch.no_grad()
def assisted_generate(engine, draft, first_token, n_tokens, k, context=None, sampling=None):
    """Assisted generation of n_tokens tokens after first_token (the token at engine.host_pos; `context`: the tokens at
    positions 0 .. host_pos - 1, which a draft may use).  Each pass verifies the last token and up to min(k, 7) drafts.
    Returns (tokens, accepted) -- the n_tokens generated tokens, and per pass the number of drafts the target accepted.
    sampling=None: greedy; raises ValueError on an engine with sampling set (the greedy verify pass accepts drafts by the
    argmax).  sampling=SamplingParams: the passes run on verify_sample with that record (a None seed is drawn once), which is
    also handed to a draft that has set_sampling(); the tokens are those of sampled run() with the same record.  The engine's
    and the draft's previous sampling state is put back before returning."""
    if sampling is None:
        if getattr(engine, "sampling", None) is not None:
            raise ValueError("assisted_generate is greedy without sampling=: this engine has sampling set (pass sampling=, or "
                             "engine.set_sampling(None) first)")
        engine.greedy = True
        return _assisted_loop(engine, engine.verify, draft, first_token, n_tokens, k, context)
    sampling = sampling.resolved()
    coupled = hasattr(draft, "set_sampling")
    prev, prev_draft = engine.sampling, getattr(draft, "sampling", None)
    try:
        engine.set_sampling(sampling)
        if coupled:
            draft.set_sampling(sampling)
        return _assisted_loop(engine, engine.verify_sample, draft, first_token, n_tokens, k, context)
    finally:
        engine.set_sampling(prev)
        if coupled:
            draft.set_sampling(prev_draft)


def _assisted_loop(engine, verify, draft, first_token, n_tokens, k, context):
    ctx = [int(t) for t in (context if context is not None else [])] + [int(first_token)]
    out, accepted = [], []
    max_seq = engine.m.shape.max_seq
    while len(out) < n_tokens:
        room = min(k, engine.VERIFY_MAX - 1, n_tokens - len(out) - 1, max_seq - engine.host_pos - 1)
        drafts = [int(t) for t in draft.propose(ctx, room)][:room] if room > 0 else []
        n, acc = verify([ctx[-1]] + drafts)
        accepted.append(n)
        out += acc
        ctx += acc
    return out[:n_tokens], accepted
