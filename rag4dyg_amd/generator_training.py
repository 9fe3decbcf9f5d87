"""RAG generator TRAINING (``main_generator.py --do_train``, ``train/train_generator.py``) on the gfx950 kernels.

One micro-step: the one-layer graph-pooling fusion forward (``r4d_weighted_bag_f32``: P = c^T X per query, then the GCN
projection ``P W^T + b``), ONE library call for the spliced GPT-2 step (``r4d_rag_train_step_f32``: forward, LM head, shifted
cross entropy over the augmented labels, backward; ``csrc/rag_train.hip``), then the fusion backward (``r4d_weight_grad_f32`` for
dW and db, and -- when wte trains -- dP = dH W and the weighted scatter ``r4d_embedding_scatter_f32``).

``--freeze`` (every shipped generator script) follows ``load_and_freeze_params`` (``utils/model.py:71-78``): the transformer is
replaced by the SimpleDyG checkpoint's, ``lm_head.weight`` keeps the model's initial wte as a separate Parameter (untied) and the
trainable set is exactly ``lm_head.weight`` + ``gnn_fusion.*``.  Gradients still run back through the frozen transformer (dropout
on: ``model.train()``) to the spliced row.  Dropout draws its masks from the library's counter-based generator, not torch's RNG.

Deviation: the bag is formed before the projection, ``(c^T X) W^T`` instead of ``c^T (X W^T)``.  Both
schedules are the reference's: ``--lrdecay 0`` the linear warm-up per optimizer step, ``--lrdecay 1`` the cosine of
``adjust_learning_rate`` before every micro-batch.  Not built: ``--fusion mlp`` training, ``--fp16``, graph pooling with
``--gnn_layers > 1`` or ``--m != 1``, ``--should_continue``: each raises.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib, gpt2, ops
from .lm_training import HeadOperand, LinearWarmupSchedule, save_checkpoint
from .training import TRAIN_HEAD_PRECISIONS, AdamW, EncoderTrainer, adjust_learning_rate, distributed_setup


# ------------------------------------------------------------------------------------------------ host preparation
def bag_weights(retrieval_sources, idxs):
    """Nodes (networkx insertion order) and pooling weights c of one query's union-of-stars graph: the one-layer GCN's
    ``mean_i (A_norm X W^T + b)_i`` equals ``(c^T X) W^T + b`` with ``c_j = (1/n) sum_i A_norm[i, j]``
    (``generator.fusion_host_prep``)."""
    from .generator import star_bag_weights
    order, c = star_bag_weights(retrieval_sources, idxs)
    return np.asarray(order, dtype=np.int64), c.astype(np.float32)


def augmented_ids(tokens, r):
    """``aug_ids`` [B, T + r]: the token ids with -100 at positions 2 .. 2 + r - 1 -- the splice, the labels
    ``cat(tok[:, :2], -100 x r, tok[:, 2:])`` of ``train_generator.py:92-95`` and the scatter ids in one array."""
    B = tokens.shape[0]
    fill = torch.full((B, r), -100, dtype=torch.int64, device=tokens.device)
    return torch.cat([tokens[:, :2].to(torch.int64), fill, tokens[:, 2:].to(torch.int64)], dim=1).contiguous()


def check_supported(args):
    """The configurations this build trains; every other one raises here, before any work."""
    if getattr(args, "fp16", False):
        raise NotImplementedError("generator training: --fp16 (apex mixed precision) is not built; the path is fp32 "
                                  "(R4D_TRAIN_PRECISION=bf16 selects this project's own mixed precision)")
    if getattr(args, "should_continue", False):
        raise NotImplementedError("generator training: --should_continue (resume) is not built")
    if args.fusion != "graphpooling":
        raise NotImplementedError(f"generator training: --fusion {args.fusion} is not built; the shipped scripts train "
                                  "--fusion graphpooling (one GCN layer, --m 1)")
    if int(args.gnn_layers) != 1:
        raise NotImplementedError("generator training: graph pooling with --gnn_layers > 1 is not built (per-query graphs, and the "
                                  "reference applies F.dropout with training=True between the layers)")
    if int(args.m) != 1:
        raise ValueError("generator training: graph pooling splices ONE row, so --m must be 1 (the reference builds T + m label "
                         "columns against T + 1 logits columns and CrossEntropyLoss raises)")


def load_and_freeze_params(model, checkpoint):
    """``utils/model.py:71-78``: the transformer's config and weights from ``checkpoint`` (a SimpleDyG ``checkpoint-0``);
    ``lm_head.weight`` keeps the model's CURRENT wte as its own Parameter (the reference's untie); the transformer is frozen."""
    from .gpt2 import GPT2Model
    dev = model.lm_head.weight.device
    model.transformer = GPT2Model.from_pretrained(checkpoint).to(dev)      # lm_head.weight stays the old Parameter: untied
    model._untied_by_checkpoint = True
    for name, p in model.named_parameters():
        if "transformer" in name:
            p.requires_grad_(False)
    gpt2.note_raw_parameter_write()
    return model


def trainable_names(model, freeze):
    """The reference's trainable set in ``named_parameters()`` order: everything, or -- under ``--freeze`` -- every name without
    ``transformer`` (``lm_head.weight`` untied, ``gnn_fusion.*``)."""
    seen, names = set(), []
    for n, p in model.named_parameters():
        if id(p) in seen or (freeze and "transformer" in n):
            continue
        seen.add(id(p))
        names.append(n)
    return names


# ------------------------------------------------------------------------------------------------ the step
class GeneratorTrainer:
    """One generator training micro-step on the device for a ``GPT2LMHeadModelRAG`` with ``gnn_fusion`` (one layer).  ``grads``
    maps the trainable names to views of ONE flat buffer (the clip norm is one launch, the data-parallel mean one all-reduce)."""

    def __init__(self, model, freeze, dropout=None, seed=0, **modes):
        """``modes``: the mode keywords of :class:`training.EncoderTrainer` and ``head_precision`` (``training.TRAIN_MODE_AXES``), handed
        to the encoder trainer unopened: it keeps the value (``self.modes``) and sets all seven switches."""
        gnn = getattr(model, "gnn_fusion", None)
        if gnn is None or gnn.n_layers != 1:
            raise _lib.R4DError("GeneratorTrainer: needs a one-layer gnn_fusion (graph pooling)")
        tied = model.lm_head.weight is model.transformer.wte.weight
        if freeze and tied:
            raise _lib.R4DError("GeneratorTrainer: --freeze needs the untied head of load_and_freeze_params")
        self.model, self.freeze, self.tied = model, bool(freeze), tied
        # layer copies / planes and the dropout struct, built once; no gradient buffer of its own
        self.enc = EncoderTrainer(model, dropout=dropout, seed=seed, want_grads=False, head=True, **modes)
        self.params = {n: p for n, p in model.named_parameters() if n in set(trainable_names(model, freeze))}
        offs, total = {}, 0
        for n, p in self.params.items():
            offs[n] = total
            total += (p.numel() + 63) // 64 * 64
        dev = model.lm_head.weight.device
        self.flat_grads = torch.zeros(total, dtype=torch.float32, device=dev)
        self.grads = {n: self.flat_grads[offs[n]:offs[n] + p.numel()].view_as(p) for n, p in self.params.items()}
        if not self.freeze:                                              # the transformer's gradients: views of the flat buffer
            self.enc.grads = {n: self.grads[n] for n in self.enc.params}
        self.flat_accum = None
        wte = model.transformer.wte.weight
        self.V, self.d = int(wte.shape[0]), int(wte.shape[1])
        self.head = HeadOperand(self.V, self.d, dev, self.enc.use_s3, self.enc.use_h2, TRAIN_HEAD_PRECISIONS[self.head_precision] == 1)
        self.ldV = self.head.ldV
        self._ws = None
        self._scratch = {}
        self._stamp = None
        ops.range_flag(dev)
        self._refresh_head()

    modes = property(lambda self: self.enc.modes)
    head_precision = property(lambda self: self.enc.head_precision)

    def select_modes(self):
        """All seven switches (process-wide: before every size query and step call)."""
        self.enc.select_modes()

    # ---------------------------------------------------------------- derived operands
    def _current_stamp(self):
        return (gpt2._RAW_WRITE_GENERATION[0], self.model.lm_head.weight._version, self.model.transformer.wte.weight._version)

    @torch.no_grad()
    def _refresh_head(self):
        """The padded head operand and its planes from ``lm_head.weight`` (== wte when tied); the transformer's copies / planes
        too unless it is frozen (built once in ``EncoderTrainer.__init__`` then)."""
        if not self.freeze and self._stamp is not None:
            self.enc.refresh_transposed()
        self.head.refresh(self.model.lm_head.weight)
        self._stamp = self._current_stamp()

    def _buf(self, key, shape, dtype=torch.float32):
        t = self._scratch.get(key)
        if t is None or tuple(t.shape) != tuple(shape):
            t = torch.empty(shape, dtype=dtype, device=self.head.pad.device)
            self._scratch[key] = t
        return t

    # ---------------------------------------------------------------- fusion
    @torch.no_grad()
    def fusion_forward(self, bags):
        """Fused rows [B, 1, d] of prepared bags ``(nodes, c, offsets, row_of)`` (``batch_bags``): P = c^T wte[nodes] per query
        (one launch), then the GCN projection P W^T + b on the GEMM.  Returns (fused, P)."""
        nodes, c, offs, _row_of = bags
        B = int(offs.numel()) - 1
        wte = self.model.transformer.wte.weight
        P = self._buf("P", (B, self.d))
        _lib.check(_lib.load().r4d_weighted_bag_f32(wte.data_ptr(), self.V, self.d, nodes.data_ptr(), c.data_ptr(), offs.data_ptr(), B,
                                                     P.data_ptr(), torch.cuda.current_stream().cuda_stream), "weighted_bag")
        conv = self.model.gnn_fusion.convs[0]
        W = conv.lin.weight                                              # [out, in]
        H = ops.conv1d(P, W.t().contiguous(), conv.bias, "none", None, W)
        return H.view(B, 1, self.d), P

    @torch.no_grad()
    def fusion_backward(self, bags, P, d_fused):
        """dW = dH^T P, db = column sums of dH (one weight-gradient launch), and -- when wte trains -- dP = dH W scattered into
        the wte gradient with the bag weights, after the token scatter and the tied head's part."""
        lib = _lib.load()
        stream = torch.cuda.current_stream().cuda_stream
        B = P.shape[0]
        dH = d_fused.view(B, self.d)
        conv = self.model.gnn_fusion.convs[0]
        dWt = self._buf("dWt", (self.d, self.d))                          # [in, out]
        ws = ops.workspace(lib.r4d_weight_grad_workspace_bytes(B, self.d, self.d), dH.device, "gen_wgrad")
        _lib.check(lib.r4d_weight_grad_f32(P.data_ptr(), dH.data_ptr(), B, self.d, self.d, dWt.data_ptr(),
                                           self.grads["gnn_fusion.convs.0.bias"].data_ptr(), ws.data_ptr(), ws.numel(), stream),
                   "weight_grad")
        self.grads["gnn_fusion.convs.0.lin.weight"].copy_(dWt.t())
        if self.freeze:
            return
        nodes, c, _offs, row_of = bags
        dP = ops.conv1d(dH, conv.lin.weight.contiguous(), None)          # [B, in] = dH [B, out] . W [out, in]
        part = self._buf("dwte_fusion", (self.V, self.d))
        ws = ops.workspace(lib.r4d_embedding_scatter_workspace_bytes(self.V, self.d), dH.device, "gen_scatter")
        _lib.check(lib.r4d_embedding_scatter_f32(dP.data_ptr(), row_of.data_ptr(), c.data_ptr(), nodes.data_ptr(), int(nodes.numel()),
                                                 self.d, self.V, part.data_ptr(), ws.data_ptr(), ws.numel(), stream), "embedding_scatter")
        self.grads["transformer.wte.weight"].add_(part)

    # ---------------------------------------------------------------- one micro-step
    @torch.no_grad()
    def step(self, tokens, bags, grad_scale=1.0, backward=True, hidden_out=None):
        """Fusion forward, the spliced step, fusion backward for one right-padded token batch [B, T] on the device.  Returns the
        loss (0-d device tensor); ``grads`` holds ``grad_scale`` * dLoss/dparameter (overwritten).  ``backward=False``: loss
        only (``evaluate()``).  ``hidden_out`` [B, T + 1, d]: receives the ln_f output rows."""
        if self._stamp != self._current_stamp():
            self._refresh_head()
        tokens = tokens.to(torch.int64)
        B, T = int(tokens.shape[0]), int(tokens.shape[1])
        fused, P = self.fusion_forward(bags)
        aug = augmented_ids(tokens, 1)
        Ta = T + 1
        lib = _lib.load()
        c, w, g, keep = self.enc._structs()
        if self.freeze or not backward:
            g = None                                                     # frozen transformer / forward only
        head = self.head.struct()
        self.select_modes()                                        # before the size query: the step call below reads the same mode
        nbytes = lib.r4d_rag_train_workspace_bytes(ctypes.byref(c), B, Ta, self.ldV)
        if nbytes == 0:
            raise _lib.R4DError("rag train step: bad batch shape")
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=tokens.device)
        loss = torch.empty((), dtype=torch.float32, device=tokens.device)
        d_fused = self._buf("d_fused", (B, 1, self.d)) if backward else None
        if backward:
            mode = _lib.HEAD_GRAD_TIED if self.tied else _lib.HEAD_GRAD_UNTIED
        else:
            mode = _lib.HEAD_GRAD_NONE
        head_grad = self.grads["lm_head.weight"] if backward and not self.tied else None
        self.enc.step += 1
        drop = self.enc._dropout_struct() if backward else None
        _lib.check(lib.r4d_rag_train_step_f32(ctypes.byref(c), ctypes.byref(w), ctypes.byref(g) if g is not None else None,
                                              ctypes.byref(head), mode, head_grad.data_ptr() if head_grad is not None else None,
                                              aug.data_ptr(), fused.contiguous().data_ptr(), B, Ta, 1, float(grad_scale), loss.data_ptr(),
                                              d_fused.data_ptr() if d_fused is not None else None,
                                              hidden_out.data_ptr() if hidden_out is not None else None,
                                              ctypes.byref(drop) if drop is not None else None, self._ws.data_ptr(), self._ws.numel(),
                                              torch.cuda.current_stream().cuda_stream), "rag_train_step")
        if backward:
            self.fusion_backward(bags, P, d_fused)
        return loss

    def accumulate(self):
        if self.flat_accum is None:
            self.flat_accum = torch.zeros_like(self.flat_grads)
        self.flat_accum.add_(self.flat_grads)

    def take_accumulated(self):
        if self.flat_accum is not None:
            self.flat_grads.copy_(self.flat_accum)
            self.flat_accum.zero_()

    def all_reduce_mean(self):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(self.flat_grads)
            self.flat_grads.div_(dist.get_world_size())


# ------------------------------------------------------------------------------------------------ data
class PreparedBags:
    """The graph preparation of every sample of a dataset, once at load: nodes and bag weights c per sample."""

    def __init__(self, index_lists, retrieval_sources, top_k):
        self.items = [bag_weights(retrieval_sources, [int(v) for v in ix][:top_k]) for ix in index_lists]

    def batch(self, sample_ids, device):
        """(nodes int64, c f32, offsets int32 [B + 1], row_of int32) on ``device`` for the samples of one batch."""
        nodes = [self.items[int(i)][0] for i in sample_ids]
        cs = [self.items[int(i)][1] for i in sample_ids]
        offs = np.zeros(len(nodes) + 1, dtype=np.int32)
        offs[1:] = np.cumsum([len(n) for n in nodes])
        row_of = np.repeat(np.arange(len(nodes), dtype=np.int32), [len(n) for n in nodes])
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device, non_blocking=True)
        return to(np.concatenate(nodes)), to(np.concatenate(cs)), to(offs), to(row_of)


class _Indexed(torch.utils.data.Dataset):
    def __init__(self, ds):
        self.ds = ds

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, i):
        return i, self.ds[i][0]


def get_dataloader(dataset, tokenizer, args, split="train"):
    """``dataloader/generator.py:105-135``: right-padded token batches (pad id), ``drop_last=True``; ``RandomSampler`` (or a
    ``DistributedSampler`` with one process per GPU) for 'train', ``SequentialSampler`` otherwise.  Batches are (sample ids, tokens)."""
    from torch.nn.utils.rnn import pad_sequence
    from torch.utils.data import DataLoader, RandomSampler, SequentialSampler

    def collate(examples):
        ids = torch.tensor([e[0] for e in examples], dtype=torch.long)
        return ids, pad_sequence([e[1] for e in examples], batch_first=True, padding_value=tokenizer.pad_token_id)

    if split == "train":
        args.train_batch_size = args.per_gpu_train_batch_size * max(1, args.n_gpu)
        bs = args.train_batch_size
        if getattr(args, "data_parallel_world", 1) <= 1:
            sampler = RandomSampler(dataset)
        else:
            from torch.utils.data.distributed import DistributedSampler
            sampler = DistributedSampler(dataset, num_replicas=int(args.data_parallel_world), rank=int(args.data_parallel_rank))
    else:
        args.eval_batch_size = args.per_gpu_eval_batch_size * max(1, args.n_gpu)
        bs = args.eval_batch_size
        sampler = SequentialSampler(dataset)
    return DataLoader(_Indexed(dataset), sampler=sampler, batch_size=bs, collate_fn=collate, drop_last=True)


# ------------------------------------------------------------------------------------------------ loop
class _OptimizerLR:
    """Under ``--lrdecay 1`` the optimizer follows ``adjust_learning_rate``; the LambdaLR exists (upstream creates it too) but is
    never stepped.  ``optimizer.pt`` records the lr the optimizer is using, as the reference's ``optimizer.state_dict()`` does."""

    def __init__(self, scheduler, optimizer):
        self.scheduler, self.optimizer = scheduler, optimizer

    @property
    def lr(self):
        return self.optimizer.lr

    def state_dict(self):
        return self.scheduler.state_dict()


def evaluate(args, trainer, loader, bags):
    """``train_generator.py:252-291``: the mean loss over the validation batches, eval mode (no dropout), forward only."""
    trainer.model.eval()
    total, n = None, 0
    for ids, tokens in loader:
        loss = trainer.step(tokens.to(args.device), bags.batch(ids, args.device), backward=False)
        total = loss if total is None else total + loss
        n += 1
    trainer.model.train()
    return float(total) / n if n else float("nan")


def train(args, train_dataset, model, tokenizer, **modes):
    """Drop-in for ``train_generator.train`` (:141-248); ``modes``: the :class:`GeneratorTrainer`'s mode keywords.  Returns
    (global_step, tr_loss / global_step)."""
    from .generator import get_eval_metrics_generator, load_and_cache_examples
    check_supported(args)
    world, rank = distributed_setup(args)
    loader = get_dataloader(train_dataset, tokenizer, args)
    bags = PreparedBags(train_dataset.index, train_dataset.retrieval_sources, args.topK)
    val_dataset = load_and_cache_examples(args, tokenizer, evaluate=True)
    val_loader = get_dataloader(val_dataset, tokenizer, args, split="eval")
    val_bags = PreparedBags(val_dataset.index, train_dataset.retrieval_sources, args.topK)
    gas = max(1, int(getattr(args, "gradient_accumulation_steps", 1)))
    if args.max_steps > 0:
        t_total = args.max_steps
        args.num_train_epochs = args.max_steps // max(1, len(loader) // gas) + 1
    else:
        t_total = len(loader) // gas * args.num_train_epochs
    trainer = GeneratorTrainer(model, freeze=bool(getattr(args, "freeze", False)),
                               seed=int(getattr(args, "seed", 0)) + 7919 * rank, **modes)
    if world > 1:
        import torch.distributed as dist
        for p in trainer.params.values():
            dist.broadcast(p.data, src=0)
        gpt2.note_raw_parameter_write()
    optimizer = AdamW(trainer.params, trainer.grads, lr=args.learning_rate, eps=args.adam_epsilon, weight_decay=args.weight_decay,
                      flat_grads=trainer.flat_grads)
    scheduler = LinearWarmupSchedule(args.learning_rate, args.warmup_steps, t_total)
    optimizer.lr = scheduler.lr
    print("***** Running training *****")
    print("  Num examples = {}".format(len(train_dataset)))
    print("  Num Epochs = {}".format(args.num_train_epochs))
    print("  Trainable parameters = {}".format(", ".join(trainer.params)))
    print("  Total optimization steps = {}".format(t_total))
    for line in trainer.modes.banner_lines():
        print(line)
    global_step, tr_loss = 0, 0.0
    best_score, best_state, best_epoch, best_step, counter = None, None, None, 0, 0
    snapshot = lambda: {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.train()
    epoch = 0
    for epoch in range(int(args.num_train_epochs)):
        model.train()
        i = 0
        for step, (ids, tokens) in enumerate(loader):
            if int(args.lrdecay) == 1:                                     # before every micro-batch, with the reference's i
                adjust_learning_rate(args, optimizer, epoch, args.learning_rate, i, len(loader))
            i += 1
            loss = trainer.step(tokens.to(args.device, non_blocking=True), bags.batch(ids, args.device), grad_scale=1.0 / gas)
            tr_loss = tr_loss + loss / gas
            if gas > 1:
                trainer.accumulate()
            if (step + 1) % gas == 0:
                if gas > 1:
                    trainer.take_accumulated()
                trainer.all_reduce_mean()
                optimizer.step(args.max_grad_norm)
                if int(args.lrdecay) == 0:
                    scheduler.step()
                    optimizer.lr = scheduler.lr
                global_step += 1
            if args.max_steps > 0 and global_step > args.max_steps:
                break
        if ops.take_range_flag() & ops.RANGE_BAD_LABEL:
            raise _lib.R4DError("generator training: a token id outside [0, vocab) reached the cross entropy")
        val_loss = evaluate(args, trainer, val_loader, val_bags)
        scores = get_eval_metrics_generator(args, epoch, model, tokenizer, global_step, mode="val", is_rag=True)
        score = scores["NDCG"][0]
        print(f"Epoch: {epoch} | Step: {global_step} | train loss: {float(tr_loss) / max(global_step, 1)} | val loss: {val_loss} | "
              f"val_NDCG@5: {score} | lr: {optimizer.lr} ")
        if epoch > args.warmup_steps:
            if best_score is None or score > best_score:
                best_score, best_state, best_epoch, best_step, counter = score, snapshot(), epoch, global_step, 0
                if rank == 0:
                    save_checkpoint(model, optimizer, scheduler if int(args.lrdecay) == 0 else _OptimizerLR(scheduler, optimizer),
                                    tokenizer, args, 0)
            else:
                counter += 1
                print("Score: {} < Best_score {}".format(score, best_score))
                print("EarlyStopping counter: {} out of {}".format(counter, args.patience))
                if counter >= args.patience:
                    print("Early Stopping.....")
                    break
    last_state, last_epoch, last_step = snapshot(), epoch, global_step
    if best_state is None:
        print(f"No epoch after the {args.warmup_steps} warm-up epochs qualified as the best model (the reference raises a "
              "NameError here): the last model stands in for it")
        best_state, best_epoch, best_step = last_state, last_epoch, last_step
    model.load_state_dict(best_state)
    print("***** Running testing *****")
    print("test_metrics best epoch : ",
          get_eval_metrics_generator(args, best_epoch, model, tokenizer, best_step, mode="test", is_rag=True, is_best=True))
    print("***** Running val *****")
    print("val_metrics best epoch : ",
          get_eval_metrics_generator(args, best_epoch, model, tokenizer, best_step, mode="val", is_rag=True, is_best=True))
    model.load_state_dict(last_state)
    print("***** Running testing on last epoch *****")
    print("test_metrics last epoch : ", get_eval_metrics_generator(args, last_epoch, model, tokenizer, last_step, mode="test", is_rag=True))
    return global_step, float(tr_loss) / max(global_step, 1)
