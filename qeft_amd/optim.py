"""The update of the training step (csrc/oweight_optim.hip): loss scaling, overflow detection,
global-norm clipping and AdamW over the oweight parameters that finetune.begin(model) returned, in two launches per step and
without a host synchronisation.

    params = finetune.begin(model)
    opt = OWeightAdamW(params)                     re-homes every oweight into one flat fp32 arena (p) with g, m, v beside it
    loss = finetune.train_step(model, opt, batches)          or by hand:
        opt.zero_grad()
        opt.scale_loss(causal_lm_loss(...), accum=k).backward()     k micro-batches sum into g
        opt.step()
    finetune.end(model)

The arena: one fp32 tensor holds every parameter in the order given, each starting at a multiple of 64 elements, the gaps zero.
`param.data` becomes a view into it and `param.grad` a view into the equally laid-out g, so the Parameter objects keep their
identity (ql.oweight, refresh_interleaved, replace_oweight, save_finetuned and end work unchanged), autograd accumulates straight
into g, and the kernels see four flat arrays: no pointer table.  Padding is zero in all four arenas and stays zero (the update of
(0, 0, 0, 0) is 0).

The state lives on the device in two 32-byte records (scale, step, good_steps, skipped_last, n_skipped, grad_norm, clip_coef,
reserved; csrc/oweight_optim.h); a step reads one and writes the other and this object swaps them.  opt.scale is a 0-d view of the
current record's scale: scale_loss multiplies by it on the device, the head's backward hands it on as a device vector, and the
update divides it out again -- no .item() anywhere.  A step whose gradient holds an inf or NaN changes nothing but the record
(and, with loss_scale="dynamic", halves the scale).

GPU only: there is no CPU path and no fallback to torch ops.  Arena is the bookkeeping alone and makes no launch.
"""
import torch

from . import _lib

ALIGN = 64                                   # elements: every tensor of the arena starts at a multiple of it
MAX_ELEMS = 2 ** 31 - 2 ** 20
STATE_FIELDS = ("scale", "step", "good_steps", "skipped_last", "n_skipped", "grad_norm", "clip_coef", "reserved")
_FLOAT_FIELDS = ("scale", "grad_norm", "clip_coef")


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def arena_layout(shapes):
    """(offsets, n) for tensors of these shapes laid out in order, each at a multiple of ALIGN elements; n is the arena's length,
    itself a multiple of ALIGN."""
    offsets, n = [], 0
    for shape in shapes:
        numel = 1
        for d in shape:
            numel *= int(d)
        offsets.append(n)
        n += (numel + ALIGN - 1) // ALIGN * ALIGN
    return offsets, n


class Arena:
    """The four flat arenas and their bookkeeping; no launch, any device.  Refuses with ValueError, before anything is touched, a
    parameter that is not an fp32, contiguous, grad-requiring leaf tensor, one that is listed twice, parameters on more than one
    device, an empty list or more than 2^31 - 2^20 elements."""

    def __init__(self, params):
        params = list(params)
        if not params:
            raise ValueError("no parameters: pass what finetune.begin(model) returned")
        for i, q in enumerate(params):
            if not torch.is_tensor(q):
                raise ValueError(f"parameter {i} is not a tensor")
            if q.dtype != torch.float32:
                raise ValueError(f"parameter {i} is {q.dtype}: the oweight parameters are fp32 (finetune.begin)")
            if not q.is_contiguous():
                raise ValueError(f"parameter {i} is not contiguous")
            if not q.requires_grad or not q.is_leaf:
                raise ValueError(f"parameter {i} does not require grad (or is not a leaf)")
            if q.device != params[0].device:
                raise ValueError(f"parameter {i} is on {q.device}, parameter 0 on {params[0].device}: one arena, one device")
        if len({id(q) for q in params}) != len(params):
            raise ValueError("a parameter is listed twice")
        self.shapes = [tuple(q.shape) for q in params]
        self.offsets, self.n = arena_layout(self.shapes)
        if self.n > MAX_ELEMS:
            raise ValueError(f"{self.n} elements exceed the arena's ceiling of 2^31 - 2^20")
        self.params = params
        dev = params[0].device
        self.p, self.g, self.m, self.v = (torch.zeros(self.n, dtype=torch.float32, device=dev) for _ in range(4))
        with torch.no_grad():
            for q, view in zip(params, self.views(self.p)):
                view.copy_(q)
                q.data = view
        for q, view in zip(params, self.views(self.g)):
            q.grad = view

    def views(self, flat):
        """The tensors of the layout as views of a flat array of n elements."""
        out = []
        for off, shape in zip(self.offsets, self.shapes):
            numel = 1
            for d in shape:
                numel *= d
            out.append(flat[off:off + numel].view(shape))
        return out

    def layout(self):
        return {"n": self.n, "shapes": [list(s) for s in self.shapes], "offsets": list(self.offsets)}

    def check_grads(self):
        """Every param.grad is still its slice of g (data_ptr alone: no synchronisation), every param.data its slice of p."""
        for i, (q, off) in enumerate(zip(self.params, self.offsets)):
            if q.grad is None or q.grad.data_ptr() != self.g.data_ptr() + 4 * off or q.grad.shape != q.shape:
                raise RuntimeError(f"the .grad of parameter {i} no longer is its slice of the gradient arena (replaced, or set to None "
                                   "by a zero_grad(set_to_none=True) from elsewhere): use this optimiser's zero_grad()")
            if q.data_ptr() != self.p.data_ptr() + 4 * off:
                raise RuntimeError(f"parameter {i} no longer lives in the arena (its .data was replaced)")

    def zero_grad(self):
        self.g.zero_()

    def load_moments(self, sd):
        """m and v of a state_dict() saved over an equally laid-out arena; ValueError, before anything is written, for another
        layout or for arrays that are not fp32 [n]."""
        if sd.get("layout") != self.layout():
            raise ValueError("the state was saved for another layout (shapes, offsets or length differ)")
        m, v = sd["m"], sd["v"]
        if m.shape != (self.n,) or v.shape != (self.n,) or m.dtype != torch.float32 or v.dtype != torch.float32:
            raise ValueError("m and v must be fp32 [n]")
        self.m.copy_(m)
        self.v.copy_(v)


def _need_gpu(params):
    for i, q in enumerate(params):
        if torch.is_tensor(q) and not q.is_cuda:
            raise RuntimeError(f"OWeightAdamW needs GPU parameters (there is no CPU path): parameter {i} is on {q.device}")


class OWeightAdamW:
    """Clipped, loss-scaled AdamW over every oweight in two launches (qeft_oweight_grad_stats, qeft_oweight_adamw).

    params: what finetune.begin(model) returned, all of them; the constructor re-homes them (Arena) or refuses: ValueError for what
    Arena refuses, RuntimeError for CPU parameters (there is no CPU path).  max_grad_norm: torch's clip_grad_norm_ over all
    parameters together, 0 turns it off.  loss_scale: "dynamic" (init_scale, halved on a non-finite step, multiplied by
    growth_factor after growth_interval applied steps), None (1) or a float; a non-finite step is skipped in every mode."""

    def __init__(self, params, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=0.3, loss_scale="dynamic",
                 init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        params = list(params)
        if not (lr >= 0 and 0 <= betas[0] < 1 and 0 <= betas[1] < 1 and eps > 0 and weight_decay >= 0 and max_grad_norm >= 0):
            raise ValueError("lr, weight_decay, max_grad_norm >= 0, betas in [0, 1) and eps > 0 are required")
        if not (growth_factor > 0 and backoff_factor > 0 and int(growth_interval) >= 1):
            raise ValueError("growth_factor, backoff_factor > 0 and growth_interval >= 1 are required")
        if loss_scale is None:
            scale, self.dynamic = 1.0, False
        elif loss_scale == "dynamic":
            scale, self.dynamic = float(init_scale), True
        elif isinstance(loss_scale, (int, float)) and not isinstance(loss_scale, bool):
            scale, self.dynamic = float(loss_scale), False
        else:
            raise ValueError(f"loss_scale must be 'dynamic', None or a number, got {loss_scale!r}")
        if not (scale > 0 and scale < float("inf")):
            raise ValueError(f"the loss scale must be positive and finite, got {scale}")
        _need_gpu(params)
        self.lr, self.betas, self.eps, self.weight_decay, self.max_grad_norm = float(lr), (float(betas[0]), float(betas[1])), \
            float(eps), float(weight_decay), float(max_grad_norm)
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self.arena = Arena(params)
        dev = self.arena.p.device
        lib = _lib.lib()
        self._blocks = lib.qeft_oweight_optim_blocks(self.arena.n)
        if self._blocks < 1:
            raise ValueError(f"the kernels refuse an arena of {self.arena.n} elements")
        self._partials = torch.zeros(self._blocks, dtype=torch.float32, device=dev)
        # two records of 8 words side by side; _cur indexes the one the next step reads
        self._records = torch.zeros(2, 8, dtype=torch.int32, device=dev)
        first = torch.zeros(8, dtype=torch.int32)
        first.view(torch.float32)[0] = scale
        first.view(torch.float32)[6] = 1.0
        self._records[0].copy_(first)
        self._cur = 0

    # ---- what a caller reads
    @property
    def params(self):
        return self.arena.params

    @property
    def scale(self):
        """The current loss scale: a 0-d fp32 device view of the current record, never a host number."""
        return self._records[self._cur].view(torch.float32)[0]

    def scale_loss(self, loss, accum=1):
        """loss * scale * (1 / accum), the scale taken on the device: backward() of the result leaves scale * d(mean loss) in g when
        `accum` micro-batches are summed."""
        return loss * self.scale * (1.0 / accum)

    def zero_grad(self):
        """One zero_() of the gradient arena; the .grad views stay what they are."""
        self.arena.zero_grad()

    def step(self, lr=None):
        """Two launches, no host synchronisation, nothing read back.  lr overrides the constructor's for this step.  Raises when a
        .grad no longer is its slice of the gradient arena."""
        a = self.arena
        a.check_grads()
        lib, st = _lib.lib(), _stream(a.p.device)
        s_in, s_out = self._records[self._cur].data_ptr(), self._records[1 - self._cur].data_ptr()
        _lib.check(lib.qeft_oweight_grad_stats(a.g.data_ptr(), a.n, s_in, self._partials.data_ptr(), st))
        _lib.check(lib.qeft_oweight_adamw(a.p.data_ptr(), a.g.data_ptr(), a.m.data_ptr(), a.v.data_ptr(), a.n, s_in, s_out,
                                          self._partials.data_ptr(), self.lr if lr is None else float(lr), self.betas[0], self.betas[1],
                                          self.eps, self.weight_decay, self.max_grad_norm, self.growth_factor, self.backoff_factor,
                                          self.growth_interval, 1 if self.dynamic else 0, st))
        self._cur = 1 - self._cur

    def stats(self):
        """The current record as a dict (synchronises)."""
        return _record_dict(self._records[self._cur].cpu())

    # ---- checkpointing
    def state_dict(self):
        """m, v and the current record on the CPU, with the layout for checking."""
        return {"m": self.arena.m.cpu(), "v": self.arena.v.cpu(), "record": self._records[self._cur].cpu(),
                "layout": self.arena.layout()}

    def load_state_dict(self, sd):
        """Takes what state_dict() of an optimiser over an equally laid-out arena returned; ValueError for another layout."""
        rec = sd["record"]
        if rec.shape != (8,) or rec.dtype != torch.int32:
            raise ValueError("the record must be int32 [8]")
        self.arena.load_moments(sd)
        self._records[self._cur].copy_(rec)


def _record_dict(words):
    """The 8 words of a record (int32 CPU tensor) by field name."""
    f = words.view(torch.float32)
    return {name: (float(f[i]) if name in _FLOAT_FIELDS else int(words[i])) for i, name in enumerate(STATE_FIELDS)}
