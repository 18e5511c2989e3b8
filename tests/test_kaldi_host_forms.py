"""ss_kaldi_mfcc_packed with host pointers: the one host-pointer form that no other GPU test calls with host inputs (the fbank form
of the same wrapper is called by test_kaldi.py).  Three clips of 2, 1 and 1 frames, 3 cepstra; the sample table ends below the
samples the caller holds and `out` has rows behind the ones the table gives: the host form equals the device form bit for bit and
the rows behind keep a sentinel.  The calls without work write nothing: no clip is SS_OK, and a clip without a frame -- which this
front end rejects, so a packed call has no empty clip -- is SS_ERR_SHORT_SIGNAL."""
import ctypes as C

import numpy as np
import pytest

from test_kaldi_cpu import SS_ERR_SHORT_SIGNAL, SS_OK, gpu_case_signal, kp, make_kaldi_params, ref_sizes

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-7777.0)


def test_mfcc_packed_host_form_equals_the_device_form(ss, sslib):
    import torch

    cfg = dict(num_mel_bins=23, num_ceps=3)
    handle = ss.KaldiConfig(make_kaldi_params(sslib, **cfg))
    flen, shift, _ = ref_sizes(kp(**cfg))
    lens = [flen + shift + 1, flen + shift - 1, flen]  # 2 frames, 1 (a hop less one sample behind it), 1
    clips = [gpu_case_signal(90 + b, n, "unit") for b, n in enumerate(lens)]
    sig = np.concatenate(clips + [gpu_case_signal(99, 37, "unit")])  # 37 samples behind the table's end
    so = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    fo = np.zeros_like(so)
    assert sslib.ss_kaldi_packed_frame_offsets(C.byref(handle.params), 3, so.ctypes.data, fo.ctypes.data) == SS_OK
    assert fo.tolist() == [0, 2, 3, 4]
    rows, spare = 4, 2

    x, dso, dfo = torch.from_numpy(sig).cuda(), torch.from_numpy(so).cuda(), torch.from_numpy(fo).cuda()
    d_out = torch.full((rows + spare, 3), float(SENTINEL), dtype=torch.float32, device="cuda")
    assert sslib.ss_kaldi_mfcc_packed_device(handle.handle, x.data_ptr(), 3, dso.data_ptr(), dfo.data_ptr(), rows, d_out.data_ptr(),
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream)) == SS_OK
    torch.cuda.synchronize()
    want = d_out.cpu().numpy()
    assert (want[:rows] != SENTINEL).all() and (want[rows:] == SENTINEL).all()

    out = np.full((rows + spare, 3), SENTINEL, dtype=np.float32)
    assert sslib.ss_kaldi_mfcc_packed(handle.handle, sig.ctypes.data, 3, so.ctypes.data, out.ctypes.data) == SS_OK
    assert out.tobytes() == want.tobytes()  # the rows of the table bit for bit, the rows behind them untouched
    # the Python front on host inputs is the same call
    got, fo_front = ss.kaldi_mfcc_packed(sig[:int(so[-1])], lens, num_mel_bins=23, num_ceps=3)
    assert fo_front.tolist() == fo.tolist() and got.tobytes() == want[:rows].tobytes()

    # no clip: SS_OK; a clip without a frame: rejected before the device is touched; neither writes anything
    untouched = np.full((rows + spare, 3), SENTINEL, dtype=np.float32)
    assert sslib.ss_kaldi_mfcc_packed(handle.handle, sig.ctypes.data, 0, so.ctypes.data, untouched.ctypes.data) == SS_OK
    short = np.array([0, lens[0], lens[0] + flen - 1, lens[0] + 2 * flen - 1], dtype=np.int64)
    assert sslib.ss_kaldi_mfcc_packed(handle.handle, sig.ctypes.data, 3, short.ctypes.data, untouched.ctypes.data) == SS_ERR_SHORT_SIGNAL
    assert (untouched == SENTINEL).all()
    assert sslib.ss_kaldi_config_device_status(handle.handle) == SS_OK
