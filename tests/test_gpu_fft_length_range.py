"""The FFT length range of the library: the reference-order transform is built for 64 .. 8192 points and is the only transform
of the reference-order chains and the per-component operators. A plan of a shorter frame is still created -- it windows, frames
and pre-emphasises -- and every entry point that would transform on it returns SMILEHIP_ERR_INVALID with the length and the
range in smilehip_last_error. (The lower boundary itself, 64 points through smilehip_rfft_frames with the bits of the oracle's
rdft, is the (64, 64, 0) case of tests/test_gpu_ooura.py::test_rfft_stage_bits_equal_reference_order.)
Also: the test helper library still builds and exports the entry points the other tests load."""
import ctypes as C
import os

import numpy as np
import pytest

ERR_INVALID = -1   # SMILEHIP_ERR_INVALID (include/smilehip.h)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def refused(capi, rc):
    """rc is SMILEHIP_ERR_INVALID and the message names the length (32) and the range (64 .. 8192)"""
    msg = capi.load().smilehip_last_error().decode()
    assert rc == ERR_INVALID, (rc, msg)
    assert "32" in msg and "64" in msg, msg


@pytest.mark.gpu
def test_frame_of_32_samples_windows_and_refuses_to_transform():
    import torch
    from opensmile_amd import capi
    ctx = capi.Context(0)
    cfg = capi.mfcc12_0_d_a_config()
    cfg.force_frame_size = 32
    cfg.stage_mask = capi.STAGE_WINDOW | capi.STAGE_FFT
    plan = capi.Plan(ctx, cfg)
    assert plan.geometry.fft_size == 32
    rows, N, K = 8, 32, 17
    x = np.random.default_rng(32).standard_normal((rows, N)).astype(np.float32)
    d_x = torch.from_numpy(x).cuda()
    d_w = torch.empty_like(d_x)
    capi.window_frames(plan, d_x.data_ptr(), N, d_w.data_ptr(), N, rows)
    torch.cuda.synchronize()
    ref = (x * plan.window()[None, :]).astype(np.float32) + np.float32(cfg.win_offset)      # windower.cpp:221-229, in float
    assert np.array_equal(bits(d_w.cpu().numpy()), bits(ref))

    L = capi.load()
    d_f = torch.zeros((rows, N), dtype=torch.float32, device="cuda")
    refused(capi, L.smilehip_rfft_frames(plan._h, d_w.data_ptr(), N, d_f.data_ptr(), N, rows, None))
    d_m = torch.zeros((rows, K), dtype=torch.float32, device="cuda")
    d_a = torch.zeros((rows, N // 2), dtype=torch.float32, device="cuda")
    refused(capi, L.smilehip_acf_frames(plan._h, d_m.data_ptr(), K, d_a.data_ptr(), N // 2, N // 2, rows, 0, 0, 0, 0, None))
    torch.cuda.synchronize()
    assert not d_f.cpu().numpy().any() and not d_a.cpu().numpy().any()         # nothing ran
    plan.close()


@pytest.mark.gpu
def test_mfcc_chain_on_a_frame_of_32_samples_is_refused_at_batch_creation():
    from opensmile_amd import capi
    ctx = capi.Context(0)
    cfg = capi.mfcc12_0_d_a_config()
    cfg.force_frame_size = 32
    cfg.n_bands = 12                      # (the 17 bins of a 32-point spectrum do not hold the file's 26 bands)
    cfg.last_mfcc = 11
    plan = capi.Plan(ctx, cfg)            # every stage's tables: the whole MFCC chain
    assert plan.geometry.fft_size == 32
    off = np.array([0, 1600, 2000], dtype=np.int64)
    h = C.c_void_p()
    refused(capi, capi.load().smilehip_batch_create(plan._h, off.ctypes.data, 2, C.byref(h)))
    assert not h.value
    plan.close()


def test_helper_library_exports_what_the_tests_load():
    p = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "libsmilehip_testkernels.so")
    assert os.path.exists(p), "tests/helpers/libsmilehip_testkernels.so not built (python __graft_entry__.py)"
    lib = C.CDLL(p)
    for name in ("log_d", "sweep_open", "sweep_close", "sweep_host", "sweep_wait", "sweep_counters", "glibc_launch", "glibc_atan2f",
                 "sqrt_launch", "div_f32_sweep", "div_f32", "div_f32_sample", "div_f64_sweep", "div_f64_sample", "f0_sw_rec"):
        assert hasattr(lib, "smilehip_debug_" + name), name
    assert not hasattr(lib, "smilehip_debug_fft_check")
