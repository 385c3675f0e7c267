"""Batched decoding: one token (greedy or sampled) for each of up to 8 independent sequences per weight pass (DESIGN.md §4.7,
§4.8).

`BatchDecodeEngine` is built on a single-GPU `DecodeEngine` (4-bit weights, v3 engine) and shares its fused operands, rotary
table and library handle, so the weights are not copied again.  It owns per-slot KV caches ([n_slots][n_kv][max_seq][128] per
layer, fp16 or -- on an engine built with kv_dtype="fp8" -- e4m3 codes with a scale per row), the per-slot
position and stop state on the device, its buffers and its graphs; it never touches the engine's own caches, position or
graphs.  One pass launches, for the m active rows (row r serves slot rows[r]): the batched token begin, per layer the verify pass's m-row linears with the batched attention between them (each row in its own slot at its own position),
the m-row head and the batched token end, which stops a row on the device when it emits its EOS token or reaches its length
limit.  A stopped row keeps its position, cache and token; later passes of the same graph leave it alone.

A sequence's tokens are the argmax of its prompt's last logits (what prefill + DecodeEngine give) followed by one token per
pass; it holds at most `max_new_tokens` of them: its length limit is position min(prompt length + max_new_tokens - 1, max_seq).
A sequence admitted with SamplingParams (qeft_amd/sampling.py) draws its tokens instead, the first one from the prompt's last
logits at position T (the prompt's length), each later one on the device at the position it will occupy; greedy and sampled
sequences share passes.
"""
import collections
import os
import types

import torch

from . import _lib, llama
from .sampling import SamplingParams, sample

REASONS = {1: "eos", 2: "length"}       # the device's done codes


def batch_unsupported(engine):
    """Why `engine` cannot serve batched decoding (the m-row pass's conditions, which the verify pass shares: one GPU, 4-bit
    weights, v3 engine; the KV cache type is the verify pass's own condition), or None."""
    why = (getattr(engine, "_m_row_unsupported", None) or engine._verify_unsupported)()
    return why.replace("the verify pass", "batched decoding") if why else None


def length_limit(prompt_len, max_new_tokens, max_seq):
    """The position at which a sequence stops for length; raises ValueError when the prompt does not fit."""
    if prompt_len < 1:
        raise ValueError("empty prompt")
    if prompt_len > max_seq:
        raise ValueError(f"a prompt of {prompt_len} tokens does not fit the KV cache (max_seq = {max_seq})")
    if max_new_tokens < 1:
        raise ValueError(f"max_new_tokens must be at least 1, got {max_new_tokens}")
    return min(prompt_len + max_new_tokens - 1, max_seq)


def stop_code(token, pos, limit, eos):
    """The stop rule of the batched token end: 1 (EOS) if `token` is the sequence's EOS, else 2 (length) if `pos` has reached
    `limit`, else 0."""
    if eos is not None and eos >= 0 and token == eos:
        return 1
    return 2 if pos >= limit else 0


class SlotTable:
    """Host bookkeeping of the slots: which hold a sequence, its tokens, position, limit and why it finished."""

    def __init__(self, n_slots):
        self.n_slots = n_slots
        self.seq = [None] * n_slots

    def free_count(self):
        return sum(q is None for q in self.seq)

    def take(self, prompt_len, limit, eos):
        """The lowest free slot, now holding a new sequence; raises RuntimeError when every slot is taken."""
        for s, q in enumerate(self.seq):
            if q is None:
                self.seq[s] = types.SimpleNamespace(prompt_len=prompt_len, pos=prompt_len, limit=limit, eos=eos, tokens=[], reason=None)
                return s
        raise RuntimeError(f"no free slot: all {self.n_slots} slots hold a sequence (release() finished ones)")

    def get(self, slot):
        if not 0 <= slot < self.n_slots or self.seq[slot] is None:
            raise KeyError(f"slot {slot} holds no sequence")
        return self.seq[slot]

    def release(self, slot):
        self.get(slot)
        self.seq[slot] = None

    def rows(self):
        """The slots still decoding, in row order (row r of a pass serves rows()[r])."""
        return [s for s, q in enumerate(self.seq) if q is not None and q.reason is None]

    def record(self, slot, tokens, pos, code):
        """New tokens of `slot`, its position and the device's done code after them."""
        q = self.get(slot)
        q.tokens.extend(tokens)
        q.pos = pos
        if code and q.reason is None:
            q.reason = REASONS[code]

    def finished(self):
        return {s: q.reason for s, q in enumerate(self.seq) if q is not None and q.reason is not None}


class _SlotView:
    """What `llama.prefill` needs of an engine, for one slot: that slot's caches per layer, P = 1 and set_position."""
    P = 1

    def __init__(self, batch, slot):
        self.lib = batch.lib
        self.kc = [k[slot] for k in batch.kc]
        self.vc = [v[slot] for v in batch.vc]
        self.ks = [x[slot] for x in batch.ks] if batch.ks is not None else None
        self.vs = [x[slot] for x in batch.vs] if batch.vs is not None else None
        self.max_seq = batch.model.shape.max_seq
        self.position = None

    def set_position(self, t):
        if not 0 <= int(t) <= self.max_seq:
            raise ValueError(f"position {t} outside the KV cache (max_seq = {self.max_seq})")
        self.position = int(t)

    def store_kv(self, li, k, v, T, start=0):
        llama.store_kv_rows(self.lib, k, v, self.kc[li], self.vc[li], self.ks[li] if self.ks is not None else None,
                            self.vs[li] if self.vs is not None else None, T, start)


class BatchDecodeEngine:
    """Greedy or sampled decoding of up to `max_batch` (<= 8) sequences at once on `engine`'s weights.  admit() prefills a prompt into a free
    slot, step() / run(n) decode every active row, finished() / tokens() / release() report and free slots."""

    MAX_BATCH = 8
    OUT_CAP = 256          # tokens per row between two host reads of the output
    MULTI = llama.DecodeEngine.MULTI

    def __init__(self, engine, max_batch=8, use_graph=True):
        why = batch_unsupported(engine)
        if why:
            raise RuntimeError(why)
        if not 1 <= int(max_batch) <= self.MAX_BATCH:
            raise ValueError(f"max_batch must be 1..{self.MAX_BATCH}, got {max_batch}")
        self.eng, self.model = engine, engine.m
        self.lib, self.dev, self.use_graph = engine.lib, engine.dev, use_graph
        s, dev = self.model.shape, engine.dev
        M = self.n_slots = int(max_batch)
        self.table = SlotTable(M)
        i32 = dict(dtype=torch.int32, device=dev)
        self.kv_dtype = engine.kv_dtype                         # the cache type of the engine it is built on
        fp8 = self.kv_dtype == "fp8"
        caches = [llama.kv_cache_arrays(self.kv_dtype, (M,), s.n_kv_heads, s.max_seq, dev) for _ in range(s.n_layers)]
        self.kc, self.vc = [c[0] for c in caches], [c[1] for c in caches]
        self.ks, self.vs = ([c[2] for c in caches], [c[3] for c in caches]) if fp8 else (None, None)
        # per slot: pos | limit | eos | done, then the sampling records [M][8] (sampling.py); one upload per admission
        self._slot_words = torch.zeros(4 * M + 8 * M, **i32)
        self.state = self._slot_words[:4 * M].view(4, M)
        self.pos, self.limit, self.eos, self.done = self.state.unbind(0)
        self.params = self._slot_words[4 * M:].view(M, 8)
        self.sampled = [False] * M                              # per slot: a sampled sequence (temperature > 0)
        self.slot_tab = torch.zeros(M, **i32)                   # row -> slot
        self.tok = torch.zeros(M, dtype=torch.long, device=dev)         # per row: the token a pass consumes (and token end writes)
        self.tok_slot = torch.zeros(M, dtype=torch.long, device=dev)    # per slot, between runs (rows change with the table)
        self.out = torch.full((M, self.OUT_CAP), -1, dtype=torch.long, device=dev)
        self.ctr = torch.zeros(2, **i32)                        # token end's step counter and arrival count
        ws_bytes = self.lib.qeft_attn_kv8_workspace_bytes if fp8 else self.lib.qeft_attn_batch_workspace_bytes
        self.b = llama.m_row_buffers(engine, M, ws_bytes(s.n_heads, 8, M))
        self.logits_m = self.b.logits
        self.graphs = {}
        self.rows = []                                          # the row table of the last pass

    # -- slots ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def admit(self, prompt, max_new_tokens, eos_id=None, sampling=None, chunk=None):
        """Prefill `prompt` into a free slot (llama.prefill on that slot's caches) and return the slot.  Its first token is the
        argmax of the prompt's last logits, or with `sampling` (SamplingParams, temperature > 0) drawn from them at position T.
        chunk=C: the prompt runs as pieces of at most C tokens on the prompt attention kernel (llama.prefill's chunk).
        Raises RuntimeError when no slot is free, ValueError when the prompt does not fit."""
        toks = torch.as_tensor(prompt, dtype=torch.long).flatten()
        T = int(toks.numel())
        limit = length_limit(T, int(max_new_tokens), self.model.shape.max_seq)
        if sampling is not None and not isinstance(sampling, SamplingParams):
            raise TypeError(f"sampling must be a SamplingParams or None, got {type(sampling).__name__}")
        self.eng._check_fresh()
        eos = int(eos_id) if eos_id is not None else -1
        sampling = sampling.resolved() if sampling is not None else None
        drawn = sampling is not None and not sampling.greedy
        slot = self.table.take(T, limit, eos)
        try:
            view = _SlotView(self, slot)
            logits = llama.prefill(self.model, toks.to(self.dev), engine=view, chunk=chunk)
            assert view.position == T
            first = sample(logits[-1], sampling, T)[0] if drawn else torch.argmax(logits[-1])
            self.tok_slot[slot] = first
            f = int(first.item())
            code = stop_code(f, T, limit, eos)
            M = self.n_slots
            rec = sampling.record() if sampling is not None else [0] * 8
            idx = [slot, M + slot, 2 * M + slot, 3 * M + slot] + list(range(4 * M + 8 * slot, 4 * M + 8 * slot + 8))
            words = torch.tensor([idx, [T, limit, eos, code] + rec], dtype=torch.int64).to(self.dev)
            self._slot_words.index_copy_(0, words[0], words[1].int())
            self.sampled[slot] = drawn
        except BaseException:
            self.table.release(slot)
            raise
        self.table.record(slot, [f], T, code)
        return slot

    def finished(self):
        """{slot: "eos" | "length"} of the sequences that stopped and are not yet released."""
        return self.table.finished()

    def tokens(self, slot):
        """The tokens `slot`'s sequence has generated so far (the first one from its prompt included)."""
        return list(self.table.get(slot).tokens)

    def release(self, slot):
        """Free `slot` (finished or not)."""
        self.table.release(slot)
        self.state[3, slot] = 2
        self.sampled[slot] = False

    def logits(self, slot):
        """fp16 logits of `slot`'s row in the last pass."""
        return self.logits_m[self.rows.index(slot)]

    # -- passes --------------------------------------------------------------------------------------------------------------
    def _split_for(self, pos):
        return self.eng._split_for(pos)

    @torch.no_grad()
    def _launch(self, m, split, sampled=False):
        """One token of m rows: token begin -> the engine's layers (DecodeEngine._v3_layers) on m-row GEMVs with the batched
        attention between them -> final norm + head -> token end (sampled: each row draws with its slot's record; greedy rows'
        records have temperature 0, the argmax)."""
        s, lib, ck, eng, b = self.model.shape, self.lib, _lib.check, self.eng, self.b
        st = torch.cuda.current_stream(self.dev).cuda_stream
        kvd = s.n_kv_heads * s.head_dim
        nq = s.hidden + 2 * kvd
        h32, qp, rope = b.h32.data_ptr(), b.qkv.data_ptr(), b.rope.data_ptr()
        slots, pos, done = self.slot_tab.data_ptr(), self.pos.data_ptr(), self.done.data_ptr()
        ck(lib.qeft_token_begin_norm_batch(self.model.model.embed_tokens.weight.data_ptr(), self.tok.data_ptr(), eng.rope_tab.data_ptr(),
                                           slots, pos, h32, rope, self.model.model.layers[0].input_layernorm.weight.data_ptr(),
                                           b.xn.data_ptr(), b.ssq.data_ptr(), s.hidden, s.vocab, s.max_seq, self.n_slots, m, st))

        def attn(li):
            opos = eng.att_pos[li].data_ptr() if eng.att_pos[li] is not None else None
            if self.ks is not None:
                ck(lib.qeft_rope_attn_decode_kv8(qp, qp + s.hidden * 2, qp + (s.hidden + kvd) * 2, nq, rope, rope + 64 * 4, 128, m,
                                                 self.kc[li].data_ptr(), self.vc[li].data_ptr(), self.ks[li].data_ptr(),
                                                 self.vs[li].data_ptr(), slots, pos, done, opos, b.att.data_ptr(), s.hidden,
                                                 b.ws.data_ptr(), split, self.n_slots, s.n_heads, s.n_kv_heads, s.max_seq, m, st))
                return
            ck(lib.qeft_rope_attn_decode_batch(qp, qp + s.hidden * 2, qp + (s.hidden + kvd) * 2, nq, rope, rope + 64 * 4, 128, m,
                                               self.kc[li].data_ptr(), self.vc[li].data_ptr(), slots, pos, done, opos,
                                               b.att.data_ptr(), s.hidden, b.ws.data_ptr(), split, self.n_slots, s.n_heads,
                                               s.n_kv_heads, s.max_seq, m, st))
        eng._v3_layers(b, eng._lin_m(b, m, st), attn)
        eng._head(h32, b.hn, self.logits_m, m, st)
        if sampled:
            ck(lib.qeft_token_end_sample_batch(self.logits_m.data_ptr(), slots, self.tok.data_ptr(), pos, self.limit.data_ptr(),
                                               self.eos.data_ptr(), done, self.out.data_ptr(), self.ctr.data_ptr(),
                                               self.params.data_ptr(), s.vocab, self.OUT_CAP, self.n_slots, m, st))
        else:
            ck(lib.qeft_token_end_batch(self.logits_m.data_ptr(), slots, self.tok.data_ptr(), pos, self.limit.data_ptr(),
                                        self.eos.data_ptr(), done, self.out.data_ptr(), self.ctr.data_ptr(), s.vocab, self.OUT_CAP,
                                        self.n_slots, m, st))

    def _pass(self, m, split, n_tok, sampled=False):
        """n_tok passes of m rows; with graphs, one graph per (m, split, n_tok, token end), captured on first use."""
        if self.use_graph:
            key = (m, split, n_tok, "sample") if sampled else (m, split, n_tok)
            g = self.graphs.get(key)
            if g is None:
                g = self.graphs[key] = llama.capture_graph(self.dev, lambda: self._launch(m, split, sampled), n_tok,
                                                           (self.state, self.tok, self.ctr, self.out))
            g.replay()
        else:
            for _ in range(n_tok):
                self._launch(m, split, sampled)

    @torch.no_grad()
    def _decode(self, n, feed=None):
        """Up to n tokens for every active row (fewer when every row has reached its length limit); the host reads the output
        once per OUT_CAP tokens and at the end.  feed: {slot: token} consumed instead of the slots' pending tokens."""
        rows = self.table.rows()
        if not rows or n <= 0:
            return
        self.eng._check_fresh()
        m = len(rows)
        if feed:
            idx = torch.tensor(list(feed), dtype=torch.long)
            self.tok_slot[idx.to(self.dev)] = torch.tensor([int(v) for v in feed.values()], dtype=torch.long).to(self.dev)
        self.slot_tab[:m].copy_(torch.tensor(rows, dtype=torch.int32))
        sel = self.slot_tab[:m].long()
        self.tok[:m] = self.tok_slot[sel]
        self.rows = rows
        # host bound of each row's position (exact unless the row stopped at EOS): picks the attention split
        hp = {s: self.table.get(s).pos for s in rows}
        lim = {s: self.table.get(s).limit for s in rows}
        multi = self.use_graph and self.MULTI > 1 and os.environ.get("QEFT_MULTI_TOKEN_GRAPH") != "0"
        sampled = any(self.sampled[s] for s in rows)
        left = n
        while left > 0:
            self.ctr.zero_()
            chunk, t = min(left, self.OUT_CAP), 0
            while t < chunk:
                live = [s for s in rows if hp[s] < lim[s]]
                if not live:
                    break
                p = max(hp[s] for s in live)
                sp = self._split_for(p)
                k = self.MULTI if multi and chunk - t >= self.MULTI and self._split_for(p + self.MULTI - 1) == sp else 1
                self._pass(m, sp, k, sampled)
                for s in rows:
                    hp[s] = min(hp[s] + k, lim[s])
                t += k
            if t:
                self._collect(rows, t)
            left -= chunk
            if t < chunk or not any(s in self.table.rows() for s in rows):
                break
        self.tok_slot[sel] = self.tok[:m]

    def _collect(self, rows, n_tok):
        out = self.out[:len(rows), :n_tok].cpu()
        st = self.state.cpu()
        for r, s in enumerate(rows):
            self.table.record(s, [int(x) for x in out[r].tolist() if x >= 0], int(st[0, s]), int(st[3, s]))

    def step(self, feed=None):
        """One token for every active row.  feed: {slot: token} to consume instead of the slots' own last tokens (teacher
        forcing); logits(slot) then holds the row's logits."""
        self._decode(1, feed)

    def run(self, n):
        """n tokens for every active row (graphs of MULTI tokens where the attention split allows); rows stop on the device at
        EOS or at their length limit, a row at max_seq finishes with "length"."""
        self._decode(n)


def generate_batch(engine, prompts, max_new_tokens, eos_id=None, max_batch=8, use_graph=True, sampling=None):
    """Continuous batching: every prompt decoded to at most max_new_tokens tokens (stopping at eos_id), up to max_batch at a
    time; a waiting prompt is admitted as soon as a slot frees up.  sampling: None (greedy), one SamplingParams for every
    prompt (a None seed is drawn per prompt) or a list with one entry (SamplingParams or None) per prompt.  Returns the token
    lists in prompt order."""
    prompts = list(prompts)
    if not prompts:
        return []
    per = list(sampling) if isinstance(sampling, (list, tuple)) else [sampling] * len(prompts)
    if len(per) != len(prompts):
        raise ValueError(f"{len(per)} sampling entries for {len(prompts)} prompts")
    be = BatchDecodeEngine(engine, max_batch=max(1, min(int(max_batch), len(prompts))), use_graph=use_graph)
    waiting = collections.deque(enumerate(prompts))
    results, owner = [None] * len(prompts), {}
    while waiting or owner:
        while waiting and be.table.free_count():
            i, p = waiting.popleft()
            owner[be.admit(p, max_new_tokens, eos_id, sampling=per[i])] = i
        be.run(2 * be.MULTI)
        for s in list(be.finished()):
            results[owner.pop(s)] = be.tokens(s)
            be.release(s)
    return results
