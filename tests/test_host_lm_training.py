"""CPU tests of the SimpleDyG LM-training host side: the training loader, the linear warm-up schedule and its saved state, and the
size queries of the LM-head entries (pure host arithmetic: no GPU needed)."""
import ctypes
import types

import torch


class _Tok:
    pad_token, pad_token_id = "<|pad|>", 7


def _args(world=1, rank=0, bs=4):
    return types.SimpleNamespace(per_gpu_train_batch_size=bs, n_gpu=1, data_parallel_world=world, data_parallel_rank=rank)


def test_training_loader_pads_with_the_pad_id_and_drops_the_last_batch():
    from torch.utils.data import RandomSampler
    from rag4dyg_amd.lm_training import get_train_dataloader
    data = [torch.arange(1, 2 + i % 5) for i in range(10)]
    loader, args = get_train_dataloader(data, _Tok(), _args())
    assert isinstance(loader.sampler, RandomSampler) and args.train_batch_size == 4
    batches = list(loader)
    assert len(batches) == 2 and all(b.shape[0] == 4 for b in batches)        # 10 // 4, the remainder dropped
    for b in batches:
        lens = (b != 7).sum(1)
        for row, n in zip(b, lens):
            assert torch.all(row[n:] == 7) and torch.equal(row[:n], torch.arange(1, 1 + int(n)))


def test_training_loader_shards_per_rank():
    from torch.utils.data.distributed import DistributedSampler
    from rag4dyg_amd.lm_training import get_train_dataloader
    data = [torch.tensor([i + 1]) for i in range(20)]
    seen = []
    for rk in range(2):
        loader, _ = get_train_dataloader(data, _Tok(), _args(world=2, rank=rk, bs=3))
        assert isinstance(loader.sampler, DistributedSampler) and loader.sampler.rank == rk
        assert len(loader) == 3                                                    # 10 per rank // 3
        seen.append({int(x) for b in loader for x in b.view(-1)})
    assert not (seen[0] & seen[1])


def test_schedule_equals_lambdalr_and_round_trips():
    from rag4dyg_amd.lm_training import LinearWarmupSchedule, linear_warmup_lambda
    lr, w, total = 1e-3, 3, 10
    ours = LinearWarmupSchedule(lr, w, total)
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=lr)
    ref = torch.optim.lr_scheduler.LambdaLR(opt, linear_warmup_lambda(w, total))
    for s in range(14):
        want = lr * (s / w if s < w else max(0.0, (total - s) / (total - w)))
        assert abs(ours.lr - want) < 1e-15 and ours.lr == opt.param_groups[0]["lr"], s
        ours.step()
        ref.step()
    import io
    buf = io.BytesIO()
    torch.save(ours.state_dict(), buf)
    buf.seek(0)
    other = torch.optim.lr_scheduler.LambdaLR(torch.optim.SGD([{"params": [torch.zeros(1)]}, {"params": [torch.zeros(1)]}], lr=lr),
                                              linear_warmup_lambda(w, total))
    other.load_state_dict(torch.load(buf, weights_only=False))
    assert other.last_epoch == 14


def test_lm_size_queries_are_host_arithmetic():
    from rag4dyg_amd import _lib
    lib = _lib.load()
    assert lib.r4d_lm_ce_workspace_bytes(16384) >= 16384 * 4 and lib.r4d_lm_ce_workspace_bytes(0) == 0
    cfg = _lib.GPT2ConfigC(2, 6, 768, 8814, 1024, 1e-5)
    B, T, ldV = 32, 512, 8832
    need = lib.r4d_gpt2_lm_train_workspace_bytes(ctypes.byref(cfg), B, T, ldV)
    Bs, Ts = (ctypes.c_int32 * 1)(B), (ctypes.c_int32 * 1)(T)
    assert need >= lib.r4d_gpt2_train_workspace_bytes(ctypes.byref(cfg), 1, Bs, Ts) + 4 * B * T * ldV
    assert lib.r4d_gpt2_lm_train_workspace_bytes(ctypes.byref(cfg), 0, T, ldV) == 0


def test_padded_vocab():
    from rag4dyg_amd.lm_training import padded_vocab
    assert [padded_vocab(v) for v in (60, 1800, 8814, 11906, 128)] == [128, 1920, 8832, 12032, 128]
