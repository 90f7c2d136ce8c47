"""GPU: `ssl4gie_amd.Models.mae.util.misc.NativeScalerWithGradNormCount` in the reference's MAE statement sequence
(Models/mae/engine_pretrain.py:39-69): the TINY MAE loop of test_gpu_reference_loop.py::_mae_loop restated — fp32,
accum_iter = 2, 6 iterations (3 updates), ArenaAdamW — once with that test's torch-op scaler (GradScaler +
per-tensor norms, extended with clip_grad as misc.py:260-263 has it) and once with the native scaler.

Bars: losses 1e-4 (INTEGRATION.md §2's own bar for these statements); norms max(4 x the error of the reference's fp32
expression against fp64, 8 * 2^-24), the bar of test_gpu_grad_norm.py, with the fp32 expression's error measured on
the gradients the native run leaves in p.grad (the fused step does not scale them)."""
import hashlib
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl4gie_amd import _lib
    _lib.load()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _torch_op_scaler():
    """misc.py:251-271 with torch ops, as test_gpu_reference_loop.py restates it, plus the clip_grad branch"""
    _scaler = torch.cuda.amp.GradScaler()

    def loss_scaler(loss, optimizer, clip_grad=None, parameters=None, create_graph=False, update_grad=True):
        _scaler.scale(loss).backward(create_graph=create_graph)
        if not update_grad:
            return None
        _scaler.unscale_(optimizer)
        if clip_grad is not None:
            norm = torch.nn.utils.clip_grad_norm_(parameters, clip_grad)
        else:
            norm = torch.norm(torch.stack([torch.norm(p.grad.detach(), 2.0) for p in parameters
                                           if p.grad is not None]), 2.0)
        _scaler.step(optimizer)
        _scaler.update()
        return norm
    return loss_scaler


def _mae_loop(rank, world, native, clip_grad, steps=6, accum_iter=2):
    """engine_pretrain.py:39-69; world > 1: under parallel.DataParallel (main_pretrain.py:175)"""
    from functools import partial
    from oracle import mae_ref, synth
    from ssl4gie_amd.Models.mae.models_mae import MaskedAutoencoderViT
    from ssl4gie_amd.Models.mae.util import misc
    from ssl4gie_amd.optim import ArenaAdamW
    cfg = mae_ref.MAEConfig(**{**mae_ref.TINY.__dict__, "norm_pix_loss": True})
    model = MaskedAutoencoderViT(img_size=cfg.img_size, patch_size=cfg.patch_size, in_chans=cfg.in_chans,
                                 embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads,
                                 decoder_embed_dim=cfg.decoder_embed_dim, decoder_depth=cfg.decoder_depth,
                                 decoder_num_heads=cfg.decoder_num_heads, mlp_ratio=cfg.mlp_ratio,
                                 norm_layer=partial(torch.nn.LayerNorm, eps=cfg.ln_eps), norm_pix_loss=True)
    model.load_state_dict(synth.mae_state_dict(cfg, 1))
    model.cuda(0).set_precision("fp32")
    model_without_ddp = model
    if world > 1:
        from ssl4gie_amd.parallel import DataParallel
        model = DataParallel(model, device_ids=[0], find_unused_parameters=True)
    optimizer = ArenaAdamW(model_without_ddp, [p for p in model_without_ddp.parameters() if p.requires_grad],
                           lr=1.5e-4, betas=(0.9, 0.95))
    loss_scaler = misc.NativeScalerWithGradNormCount() if native else _torch_op_scaler()

    losses, reduced, returned, norms, bits, bars = [], [], [], [], [], []
    model.train(True)
    optimizer.zero_grad()
    for data_iter_step in range(steps):
        samples = synth.synth_images(4, cfg, seed=10 * rank + data_iter_step).cuda(0, non_blocking=True)
        noise = torch.from_numpy(synth.synth_noise(4, cfg.num_patches, seed=50 * rank + data_iter_step)).cuda(0)
        loss, _, _ = model(samples, mask_ratio=0.75, noise=noise)
        loss_value = loss.item()
        assert np.isfinite(loss_value)
        loss /= accum_iter
        update = (data_iter_step + 1) % accum_iter == 0
        norm = loss_scaler(loss, optimizer, clip_grad=clip_grad, parameters=model.parameters(), update_grad=update)
        returned.append(norm is not None)
        if update:
            norms.append(float(norm))
            bits.append(int(norm.detach().view(torch.int32).item()))
            if native:   # p.grad is still the unscaled gradient the norm was taken of: the bar of this update
                grads = [p.grad.detach() for p in model.parameters() if p.grad is not None]
                ref64 = torch.cat([g.double().flatten() for g in grads]).norm().item()
                fp32 = float(torch.norm(torch.stack([torch.norm(g, 2.0) for g in grads]), 2.0))
                err_torch = abs(fp32 - ref64) / ref64
                bars.append((ref64, err_torch, max(4.0 * err_torch, 8.0 * EPS)))
            optimizer.zero_grad()
        torch.cuda.synchronize()
        losses.append(loss_value)
        reduced.append(misc.all_reduce_mean(loss_value))   # engine_pretrain.py:69
    flat = torch.cat([p.detach().flatten() for p in model.parameters()])
    sig = hashlib.sha256(flat.cpu().numpy().tobytes()).hexdigest()   # every bit of every weight
    return dict(losses=losses, reduced=reduced, returned=returned, norms=norms, bits=bits, bars=bars, sig=sig,
                steps=optimizer.step_count)


def test_native_scaler_matches_the_torch_op_scaler_single_process():
    first = _mae_loop(0, 1, native=False, clip_grad=None)["norms"][0]
    clip = 0.5 * first                                   # below the first measured norm: clipping is live
    ref = _mae_loop(0, 1, native=False, clip_grad=clip)
    nat = _mae_loop(0, 1, native=True, clip_grad=clip)
    assert nat["returned"] == ref["returned"] == [False, True] * 3   # None on the non-update iterations
    assert nat["norms"][0] > clip
    assert np.allclose(nat["losses"], ref["losses"], rtol=1e-4), (nat["losses"], ref["losses"])
    for k, (n_nat, n_ref, (ref64, err_torch, bar)) in enumerate(zip(nat["norms"], ref["norms"], nat["bars"])):
        own = abs(n_nat - ref64) / ref64
        cross = abs(n_nat - n_ref) / n_ref
        print(f"update {k}: native {n_nat!r} torch-op {n_ref!r}; native vs fp64 {own:.3e}, vs the torch-op run "
              f"{cross:.3e}; fp32 expression vs fp64 {err_torch:.3e}; bar {bar:.3e}")
        assert own <= bar, (k, own, err_torch, bar)
        assert cross <= bar, (k, cross, err_torch, bar)
    assert nat["steps"] == 3
    assert nat["reduced"] == nat["losses"]   # one process: all_reduce_mean hands the number back


def test_scaler_checkpoint_round_trip():
    from ssl4gie_amd.Models.mae.util import misc
    saved = torch.cuda.amp.GradScaler().state_dict()   # what a reference checkpoint holds under "amp_scaler"
    assert saved, "GradScaler is enabled on this device"
    s = misc.NativeScalerWithGradNormCount()
    s.load_state_dict(saved)
    assert s.state_dict() == saved
    t = torch.cuda.amp.GradScaler()
    t.load_state_dict(s.state_dict())                  # and the way back: torch accepts ours
    assert t.state_dict() == saved


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), SSL4GIE_COMM_CUS="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    out = {}
    try:
        out["native"] = _mae_loop(rank, world, native=True, clip_grad=1e-3)
    except Exception:  # noqa: BLE001 - reported to the parent
        import traceback
        out["error"] = traceback.format_exc()
    q.put((rank, out))
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_native_scaler_two_ranks_one_device():
    """different data per rank, gloo between them: after the all-reduce both ranks hold the same gradient arena, and
    the fixed-order norm pass must give the same BITS on both; so the clip coefficient and the weights stay equal"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    for r in (0, 1):
        assert "error" not in res[r], res[r]["error"]
    a, b = res[0]["native"], res[1]["native"]
    assert len(a["bits"]) == 3 and a["bits"] == b["bits"], (a["norms"], b["norms"])
    assert a["sig"] == b["sig"], "the weights differ between the ranks"
    # misc.all_reduce_mean: both ranks log the same number, the mean of their losses.  It is formed in fp32 (the
    # reference builds the tensor with torch.tensor(x)): each loss rounded, one add, an exact halving: 3 EPS
    assert a["reduced"] == b["reduced"] and a["losses"] != b["losses"]
    for la, lb, red in zip(a["losses"], b["losses"], a["reduced"]):
        assert abs(red - 0.5 * (la + lb)) <= 3.0 * EPS * 0.5 * (la + lb), (la, lb, red)
    assert a["returned"] == [False, True] * 3 and a["steps"] == b["steps"] == 3
    assert all(n > 1e-3 for n in a["norms"]), a["norms"]   # the clip was live on every update
