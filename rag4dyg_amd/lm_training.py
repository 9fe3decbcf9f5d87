"""SimpleDyG LM TRAINING (``main_SimpleDyG.py --do_train``) on the gfx950 kernels: the training forward with saved activations, the
LM head (logits over every position against the tied ``wte``), the shifted cross entropy and the backward pass -- ONE library call
per micro-batch (``r4d_gpt2_lm_train_step_f32``, ``csrc/lm_head.hip``) -- then gradient accumulation, the data-parallel average,
``clip_grad_norm_`` + AdamW (``training.AdamW``) under ``get_linear_schedule_with_warmup``, per-epoch validation NDCG@5 with early
stopping, and the reference's checkpoint layout.

Mirrors ``main_SimpleDyG.py:148-343`` (``train_epoch``, ``train``), ``dataloader/SimpleDyG.py:36-53`` (the training loader) and
``utils/model.py:56-102`` (checkpoints, optimizer groups, schedule).  Dropout draws its masks from the library's counter-based
generator (``EncoderTrainer``), not torch's RNG stream; in ``model.eval()`` terms every number equals the reference's calculus.
"""
import argparse
import ctypes
import os

import torch

from . import _lib, gpt2, ops
from .training import TRAIN_HEAD_PRECISIONS, AdamW, EncoderTrainer, distributed_setup, write_checkpoint_dir


def padded_vocab(V):
    """Rows of the padded LM-head operand: V rounded up to 128 (the alignment of every GEMM family's tiles)."""
    return (int(V) + 127) // 128 * 128


def head_chunks(ldV, chunk_rows):
    """The vocabulary chunks of the LM head as (first row, rows): ``[k C, min((k + 1) C, ldV))`` for ``C = chunk_rows`` (the
    library's ``r4d_lm_head_chunk_rows(ldV)``: ldV itself up to 15,872 rows, a fixed multiple of 128 beyond).  The last chunk may
    be shorter; with ldV a multiple of 128 every chunk is one."""
    ldV, C = int(ldV), int(chunk_rows)
    if ldV < 1 or C < 1 or ldV % 128 or (C % 128 and C != ldV):
        raise ValueError(f"head_chunks: ldV={ldV} chunk_rows={C} (multiples of 128 wanted)")
    return [(c0, min(C, ldV - c0)) for c0 in range(0, ldV, C)]


class HeadOperand:
    """The padded LM-head operand ``pad`` [ldV, d] (the head weight in rows [0, V), zero rows up to ldV) and its GEMM planes, as
    ``r4d_lm_head`` describes them: bf16x3 planes when the split modes are on, f16x2 planes in f16x2 mode.  Beyond 15,872 rows the
    bf16x3 planes are laid chunk by chunk (``head_chunks``: the chunked head of ``csrc/lm_head.hip``); the buffers keep their
    sizes.  ``head_bf16`` (head precision ``bf16``, ``r4d_set_train_head_bf16``): the bf16x3 planes are built in EVERY gemm mode,
    exact f32 included -- the head's GEMMs read plane 0 of them; with the switch off the library takes no route through them in
    exact-f32 mode.  Shared by the SimpleDyG and the RAG-generator training steps; ``refresh(weight)`` after every change of the
    head weight."""

    def __init__(self, V, d, device, use_s3, use_h2, head_bf16=False):
        self.V, self.d, self.ldV = int(V), int(d), padded_vocab(V)
        self.pad = torch.zeros(self.ldV, self.d, dtype=torch.float32, device=device)
        self._w3 = self._w3t = self._h2 = None
        if (use_s3 or head_bf16) and self.d % 32 == 0:
            self._w3 = torch.empty(3, self.ldV, self.d, dtype=torch.int16, device=device)       # one chunk: this shape; else per chunk
            self._w3t = torch.empty(3, self.d, self.ldV, dtype=torch.int16, device=device)
            if use_h2:
                self._h2 = torch.empty(self.ldV, self.d // 32, 2, 32, dtype=torch.int16, device=device)

    @torch.no_grad()
    def refresh(self, weight):
        self.pad[:self.V].copy_(weight)
        if self._w3 is not None:
            lib = _lib.load()
            stream = torch.cuda.current_stream().cuda_stream
            p = self.pad.data_ptr()
            for c0, cn in head_chunks(self.ldV, lib.r4d_lm_head_chunk_rows(self.ldV)):
                w, planes = p + 4 * c0 * self.d, 2 * 3 * c0 * self.d          # byte offsets of the chunk's rows / its planes
                _lib.check(lib.r4d_split3_planes_bf16(w, self.d, cn, 1, self._w3.data_ptr() + planes, stream), "split3_planes")
                _lib.check(lib.r4d_split3_planes_bf16(w, cn, self.d, 0, self._w3t.data_ptr() + planes, stream), "split3_planes")
            if self._h2 is not None:
                _lib.check(lib.r4d_split2_planes_f16(p, self.d, self.ldV, 1, self._h2.data_ptr(), stream), "split2_planes")

    def struct(self):
        h2 = self._h2 is not None and ops.gemm_mode() == "f16x2"
        return _lib.LMHeadC(self.pad.data_ptr(), self.ldV, self._w3.data_ptr() if self._w3 is not None else None,
                            self._w3t.data_ptr() if self._w3t is not None else None, self._h2.data_ptr() if h2 else None)


@torch.no_grad()
def lm_head_train(head, h, labels_src, T, grad_scale=1.0, dh=None, dwte=None, workspace=None):
    """The LM head of the two training steps alone (``r4d_lm_head_train_f32``), in the CURRENT gemm mode and head switch
    (``r4d_set_train_head_bf16``): ``head`` a refreshed :class:`HeadOperand`, ``h`` fp32 [N, d] on the device (N = B T rows),
    ``labels_src`` int64 [N] (the label of row r is ``labels_src[r + 1]`` inside a sequence of T rows; -100 is not counted).
    ``dh`` [N, d] / ``dwte`` [ldV, d]: written when given (``grad_scale`` * gradient); both None: the loss alone.  ``workspace``: a
    uint8 device tensor of at least ``r4d_lm_head_train_workspace_bytes`` (None: a fresh one).  Returns (loss, workspace)."""
    lib = _lib.load()
    N, d = int(h.shape[0]), int(h.shape[1])
    for t, n in ((h, "h"), (dh, "dh"), (dwte, "dwte")):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous()):
            raise _lib.R4DError(f"lm_head_train: {n} must be a contiguous fp32 device tensor")
    if d != head.d or not labels_src.is_cuda or labels_src.dtype != torch.int64 or labels_src.numel() != N:
        raise _lib.R4DError("lm_head_train: h is [N, head.d], labels_src int64 [N] on the device")
    nbytes = int(lib.r4d_lm_head_train_workspace_bytes(N, d, head.ldV))
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=h.device)
    loss = torch.empty((), dtype=torch.float32, device=h.device)
    st = head.struct()
    _lib.check(lib.r4d_lm_head_train_f32(h.data_ptr(), N, head.V, d, ctypes.byref(st), labels_src.data_ptr(), int(T), float(grad_scale),
                                         loss.data_ptr(), dh.data_ptr() if dh is not None else None,
                                         dwte.data_ptr() if dwte is not None else None, workspace.data_ptr(), workspace.numel(),
                                         torch.cuda.current_stream().cuda_stream), "lm_head_train")
    return loss, workspace


class LMTrainer:
    """One SimpleDyG training micro-step on the device.  Built on :class:`training.EncoderTrainer` (the flat gradient buffer,
    the per-layer weight copies / planes, the dropout struct, ``accumulate`` / ``take_accumulated`` / ``all_reduce_mean``) plus
    the padded LM-head operand ``wte_pad`` [ldV, d] (zero rows past V) and its planes.  Every derived weight is rebuilt when the
    parameters changed since the last step (``gpt2.note_raw_parameter_write`` generation, or torch's version counter of wte)."""

    def __init__(self, model, dropout=None, seed=0, **modes):
        """``modes``: the mode keywords of :class:`training.EncoderTrainer` and ``head_precision`` (``training.TRAIN_MODE_AXES``), handed
        to the encoder trainer unopened: it keeps the value (``self.modes``) and sets all seven switches, the head's with the others,
        before every size query and step call."""
        head = getattr(model, "lm_head", None)
        if head is None or head.weight is not model.transformer.wte.weight:
            raise _lib.R4DError("SimpleDyG training needs lm_head tied to transformer.wte (the reference's model is always tied); "
                                "this model's lm_head is a separate tensor")
        self.model = model
        self.enc = EncoderTrainer(model, dropout=dropout, seed=seed, head=True, **modes)
        wte = self.enc.params["transformer.wte.weight"]
        V, d = wte.shape
        self.V, self.d, self.ldV = int(V), int(d), padded_vocab(V)
        dev = wte.device
        self.head = HeadOperand(V, d, dev, self.enc.use_s3, self.enc.use_h2, TRAIN_HEAD_PRECISIONS[self.head_precision] == 1)
        self._ws = None
        self._stamp = None
        ops.range_flag(dev)                                     # registered: the CE kernel reports out-of-range labels there
        self.refresh()

    modes = property(lambda self: self.enc.modes)
    head_precision = property(lambda self: self.enc.head_precision)

    def select_modes(self):
        """All seven switches (process-wide: before every size query and step call)."""
        self.enc.select_modes()

    # the EncoderTrainer surface the training loop uses
    @property
    def params(self):
        return self.enc.params

    @property
    def grads(self):
        return self.enc.grads

    @property
    def flat_grads(self):
        return self.enc.flat_grads

    def accumulate(self):
        self.enc.accumulate()

    def take_accumulated(self):
        self.enc.take_accumulated()

    def all_reduce_mean(self):
        self.enc.all_reduce_mean()

    def _current_stamp(self):
        return (gpt2._RAW_WRITE_GENERATION[0], self.enc.params["transformer.wte.weight"]._version)

    @torch.no_grad()
    def refresh(self):
        """Bring the layer copies / planes and the LM-head operand and planes up to date with the parameters."""
        self.enc.refresh_transposed()
        self.head.refresh(self.enc.params["transformer.wte.weight"])
        self._stamp = self._current_stamp()

    @torch.no_grad()
    def step(self, ids, grad_scale=1.0):
        """Forward, shifted cross entropy (labels == inputs) and backward over one right-padded id batch [B, T] on the device.
        Returns the loss (0-d device tensor, not scaled); ``grads`` holds ``grad_scale`` * dLoss/dparameter (overwritten)."""
        if self._stamp != self._current_stamp():
            self.refresh()
        ids = ids.to(torch.int64).contiguous()
        if ids.dim() != 2 or not ids.is_cuda:
            raise _lib.R4DError("LMTrainer.step: ids must be a [B, T] device tensor")
        B, T = int(ids.shape[0]), int(ids.shape[1])
        lib = _lib.load()
        c, w, g, keep = self.enc._structs()
        head = self.head.struct()
        self.select_modes()                                  # before the size query: the step call below reads the same mode
        nbytes = lib.r4d_gpt2_lm_train_workspace_bytes(ctypes.byref(c), B, T, self.ldV)
        if nbytes == 0:
            raise _lib.R4DError("lm train step: bad batch shape")
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=ids.device)
        loss = torch.empty((), dtype=torch.float32, device=ids.device)
        self.enc.step += 1                                         # the dropout counter of EncoderTrainer
        drop = self.enc._dropout_struct()
        _lib.check(lib.r4d_gpt2_lm_train_step_f32(ctypes.byref(c), ctypes.byref(w), ctypes.byref(g), ctypes.byref(head), ids.data_ptr(),
                                                  B, T, float(grad_scale), loss.data_ptr(),
                                                  ctypes.byref(drop) if drop is not None else None, self._ws.data_ptr(),
                                                  self._ws.numel(), torch.cuda.current_stream().cuda_stream), "gpt2_lm_train_step")
        return loss


# ------------------------------------------------------------------------------------------------ data and schedule
def get_train_dataloader(dataset, tokenizer, args):
    """``dataloader/SimpleDyG.py:36-53``, split 'train': one right-padded tensor per batch (padded with the pad id),
    ``RandomSampler`` -- or ``DistributedSampler`` with one process per GPU --, ``drop_last=True``."""
    from torch.nn.utils.rnn import pad_sequence
    from torch.utils.data import DataLoader, RandomSampler
    pad = {} if tokenizer.pad_token is None else {"padding_value": tokenizer.pad_token_id}

    def collate(examples):
        return pad_sequence(examples, batch_first=True, **pad)

    args.train_batch_size = args.per_gpu_train_batch_size * max(1, args.n_gpu)
    if getattr(args, "data_parallel_world", 1) <= 1:
        sampler = RandomSampler(dataset)
    else:
        from torch.utils.data.distributed import DistributedSampler
        sampler = DistributedSampler(dataset, num_replicas=int(args.data_parallel_world), rank=int(getattr(args, "data_parallel_rank", 0)))
    return DataLoader(dataset, sampler=sampler, batch_size=args.train_batch_size, collate_fn=collate, drop_last=True), args


def linear_warmup_lambda(num_warmup_steps, num_training_steps):
    """``get_linear_schedule_with_warmup``'s multiplier (``utils/model.py:90-93``)."""
    def lr_lambda(step):
        if step < num_warmup_steps:
            return float(step) / float(max(1, num_warmup_steps))
        return max(0.0, float(num_training_steps - step) / float(max(1, num_training_steps - num_warmup_steps)))
    return lr_lambda


class LinearWarmupSchedule:
    """The schedule as a real ``torch.optim.lr_scheduler.LambdaLR`` (over the reference's two parameter groups, on placeholder
    parameters) so that ``scheduler.pt`` is exactly the state dict upstream saves; ``lr`` is what the device optimizer uses."""

    def __init__(self, lr, num_warmup_steps, num_training_steps):
        self._opt = torch.optim.SGD([{"params": [torch.zeros(1)]}, {"params": [torch.zeros(1)]}], lr=lr)
        self.sched = torch.optim.lr_scheduler.LambdaLR(self._opt, linear_warmup_lambda(num_warmup_steps, num_training_steps))

    @property
    def lr(self):
        return self._opt.param_groups[0]["lr"]

    def step(self):
        import warnings
        with warnings.catch_warnings():                  # the placeholder optimizer never steps: torch's order warning is moot
            warnings.simplefilter("ignore", UserWarning)
            self.sched.step()

    def state_dict(self):
        return self.sched.state_dict()


def optimizer_state_dict(optimizer, model, lr):
    """``optimizer.pt`` in the state-dict layout of a torch AdamW over the reference's two groups (``utils/model.py:80-88``:
    decayed parameters first, then ``bias`` / ``LayerNorm.weight``), parameters numbered in that order."""
    names = [n for n, _p in model.named_parameters() if n in optimizer.params]
    no_decay = ("bias", "LayerNorm.weight")
    groups = [[n for n in names if not any(nd in n for nd in no_decay)], [n for n in names if any(nd in n for nd in no_decay)]]
    state, idx, pgs = {}, 0, []
    for gi, grp in enumerate(groups):
        ids = []
        for n in grp:
            state[idx] = {"step": torch.tensor(float(optimizer.t)), "exp_avg": optimizer.m[n].detach().cpu(),
                          "exp_avg_sq": optimizer.v[n].detach().cpu()}
            ids.append(idx)
            idx += 1
        wd = optimizer.wd[grp[0]] if grp else 0.0
        pgs.append({"lr": lr, "betas": optimizer.betas, "eps": optimizer.eps, "weight_decay": wd, "params": ids})
    return {"state": state, "param_groups": pgs}


def save_checkpoint(model, optimizer, scheduler, tokenizer, args, global_step):
    """``utils/model.py:56-69``: ``<output_dir>/checkpoint-<n>/{config.json, pytorch_model.bin, tokenizer files, training_args.bin,
    optimizer.pt, scheduler.pt}``, with ``--save_total_limit`` rotation (:41-53) before the optimizer state is written."""
    out = write_checkpoint_dir(model, tokenizer, args, global_step, pack_args=argparse.Namespace)    # a Namespace, as upstream (device dropped)
    os.makedirs(out, exist_ok=True)
    torch.save(optimizer_state_dict(optimizer, model, scheduler.lr), os.path.join(out, "optimizer.pt"))
    torch.save(scheduler.state_dict(), os.path.join(out, "scheduler.pt"))


# ------------------------------------------------------------------------------------------------ training loop
def train_epoch(model, trainer, optimizer, scheduler, train_dataloader, tr_loss, global_step, args):
    """``main_SimpleDyG.py:148-198``: one pass; losses stay on the device (summed there), one optimizer update every
    ``gradient_accumulation_steps`` micro-batches; stops once ``global_step > max_steps``."""
    gas = max(1, int(getattr(args, "gradient_accumulation_steps", 1)))
    model.train()
    for step, batch in enumerate(train_dataloader):
        loss = trainer.step(batch.to(args.device, non_blocking=True), grad_scale=1.0 / gas)
        tr_loss = tr_loss + loss / gas
        if gas > 1:
            trainer.accumulate()
        if (step + 1) % gas == 0:
            if gas > 1:
                trainer.take_accumulated()
            trainer.all_reduce_mean()
            optimizer.step(args.max_grad_norm)
            scheduler.step()
            optimizer.lr = scheduler.lr
            global_step += 1
        if args.max_steps > 0 and global_step > args.max_steps:
            break
    return global_step, tr_loss


def train(args, train_dataset, model, tokenizer, **modes):
    """Drop-in for ``main_SimpleDyG.train`` (:200-343); ``modes``: the :class:`LMTrainer`'s mode keywords.  Returns (global_step,
    tr_loss / global_step)."""
    from .evaluation import get_eval_metrics
    if getattr(args, "fp16", False):
        raise NotImplementedError("SimpleDyG training: --fp16 (apex mixed precision) is not built; the path is fp32 "
                                  "(R4D_TRAIN_PRECISION=bf16 selects this project's own mixed precision)")
    world, rank = distributed_setup(args)
    train_dataloader, args = get_train_dataloader(train_dataset, tokenizer, args)
    gas = max(1, int(getattr(args, "gradient_accumulation_steps", 1)))
    if args.max_steps > 0:
        t_total = args.max_steps
        args.num_train_epochs = args.max_steps // max(1, len(train_dataloader) // gas) + 1
    else:
        t_total = len(train_dataloader) // gas * args.num_train_epochs
    trainer = LMTrainer(model, seed=int(getattr(args, "seed", 0)) + 7919 * rank, **modes)      # every rank its own dropout masks
    if world > 1:
        import torch.distributed as dist
        for p in trainer.params.values():                       # DistributedDataParallel's construction-time broadcast
            dist.broadcast(p.data, src=0)
        gpt2.note_raw_parameter_write()
    optimizer = AdamW(trainer.params, trainer.grads, lr=args.learning_rate, eps=args.adam_epsilon, weight_decay=args.weight_decay,
                      flat_grads=trainer.flat_grads)
    scheduler = LinearWarmupSchedule(args.learning_rate, args.warmup_steps, t_total)
    optimizer.lr = scheduler.lr
    print("***** Running training *****")
    print("  Num examples = {}".format(len(train_dataset)))
    print("  Num Epochs = {}".format(args.num_train_epochs))
    print("  Instantaneous batch size per GPU = {}".format(args.per_gpu_train_batch_size))
    print("  Total train batch size (w. parallel, distributed & accumulation) = {}".format(args.train_batch_size * gas * world))
    print("  Gradient Accumulation steps = {}".format(gas))
    for line in trainer.modes.banner_lines():
        print(line)
    print("  Total optimization steps = {}".format(t_total))
    global_step, tr_loss = 0, 0.0
    best_score, best_state, best_step, counter = None, None, 0, 0
    snapshot = lambda: {k: v.detach().clone() for k, v in model.state_dict().items()}     # device-side copy
    for epoch in range(int(args.num_train_epochs)):
        global_step, tr_loss = train_epoch(model, trainer, optimizer, scheduler, train_dataloader, tr_loss, global_step, args)
        if ops.take_range_flag() & ops.RANGE_BAD_LABEL:
            raise _lib.R4DError("SimpleDyG training: a token id outside [0, vocab) reached the cross entropy (corrupt ids or a "
                                "tokenizer / checkpoint vocabulary mismatch)")
        scores = get_eval_metrics(args, model, tokenizer, global_step, mode="val")
        score = scores['NDCG'][0]
        print(f"Epoch: {epoch} | Step: {global_step} | train loss: {float(tr_loss) / max(global_step, 1)}  | "
              f"val_NDCG@5: {scores['NDCG'][0]} | lr: {scheduler.lr} ")
        early_stop = False
        if best_score is not None and score < best_score:
            counter += 1
            print('Score: {} < Best_score {}'.format(score, best_score))
            print('EarlyStopping counter: {} out of {}'.format(counter, args.patience))
            early_stop = counter >= args.patience
        else:
            best_score, best_state, best_step, counter = score, snapshot(), global_step, 0
            if rank == 0:
                save_checkpoint(model, optimizer, scheduler, tokenizer, args, 0)
        if early_stop:
            print('Early Stopping.....')
            break
    if best_state is None:
        best_state, best_step = snapshot(), global_step
    model.load_state_dict(best_state)
    print("***** Running val *****")
    print('top_k_scores_val: ', get_eval_metrics(args, model, tokenizer, best_step, mode="val"))
    print("***** Running test *****")
    print('top_k_scores_test: ', get_eval_metrics(args, model, tokenizer, best_step, mode="test"))
    return global_step, float(tr_loss) / max(global_step, 1)
