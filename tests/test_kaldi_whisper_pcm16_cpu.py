"""The one-shot Kaldi and Whisper calls fed signed 16-bit PCM, without a device: the twelve entries (ss_kpcm_* and
ss_whisper_log_mel*_i16*) are exported, declared and mirrored, answer a null handle as their float twins do, and ``pcm_scale=`` of the
nine Python functions follows the rules of ``mfcc(..., pcm_scale=)`` before anything touches a device.  The bit-for-bit comparisons
with the float calls are tests/test_kaldi_pcm16.py and tests/test_whisper_pcm16.py."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_kaldi_cpu import HEADER, SS_ERR_ARG

# name -> (its float twin, the arguments behind the handle and the sample pointer, the float twin's)
_D, _P = (1, 400, 400), (1, None)
ENTRIES = {
    "ss_kpcm_fbank_device": ("ss_kaldi_fbank_device", (*_D, 1.0, None, None, None), (*_D, None, None, None)),
    "ss_kpcm_fbank": ("ss_kaldi_fbank", (*_D, 1.0, None, None), (*_D, None, None)),
    "ss_kpcm_mfcc_device": ("ss_kaldi_mfcc_device", (*_D, 1.0, None, None), (*_D, None, None)),
    "ss_kpcm_mfcc": ("ss_kaldi_mfcc", (*_D, 1.0, None), (*_D, None)),
    "ss_kpcm_fbank_packed_device": ("ss_kaldi_fbank_packed_device", (*_P, 1.0, None, 1, None, None, None), (*_P, None, 1, None, None, None)),
    "ss_kpcm_fbank_packed": ("ss_kaldi_fbank_packed", (*_P, 1.0, None, None), (*_P, None, None)),
    "ss_kpcm_mfcc_packed_device": ("ss_kaldi_mfcc_packed_device", (*_P, 1.0, None, 1, None, None), (*_P, None, 1, None, None)),
    "ss_kpcm_mfcc_packed": ("ss_kaldi_mfcc_packed", (*_P, 1.0, None), (*_P, None)),
    "ss_whisper_log_mel_i16_device": ("ss_whisper_log_mel_device", (*_D, 2.0 ** -15, 2, 0, None, None, None), (*_D, 2, 0, None, None, None)),
    "ss_whisper_log_mel_i16": ("ss_whisper_log_mel", (*_D, 2.0 ** -15, 2, 0, None), (*_D, 2, 0, None)),
    "ss_whisper_log_mel_packed_i16_device": ("ss_whisper_log_mel_packed_device", (*_P, 2.0 ** -15, 2, 0, None, None, None, None),
                                             (*_P, 2, 0, None, None, None, None)),
    "ss_whisper_log_mel_packed_i16": ("ss_whisper_log_mel_packed", (*_P, 2.0 ** -15, 2, 0, None, None), (*_P, 2, 0, None, None)),
}


def test_the_twelve_entries_are_exported_declared_and_mirrored(sslib):
    from speechsauce_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert len(ENTRIES) == 12
    for name, (twin, args, twin_args) in ENTRIES.items():
        assert name in exported, f"{name} is not exported"
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, flags=re.S)
        assert m, f"{name} is not declared"
        params = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
        assert params[1].startswith("const int16_t *"), (name, params[1])
        assert "float scale" in params, name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == len(params) == len(args) + 2, name
        assert len(_lib.PROTOTYPES[twin][1]) == len(params) - 1 == len(twin_args) + 2, twin
    assert sslib.ss_abi_version() == 7 == _lib.ABI_VERSION
    assert "#define SS_ABI_VERSION 7" in open(HEADER).read()
    # the Kaldi entries stay out of the ss_kaldi_* name set, whose members another test pins
    assert not [n for n in ENTRIES if n.startswith("ss_kaldi_")]


def test_a_null_handle_is_answered_as_by_the_float_twin(sslib):
    for name, (twin, args, twin_args) in ENTRIES.items():
        assert getattr(sslib, name)(None, None, *args) == getattr(sslib, twin)(None, None, *twin_args) == SS_ERR_ARG, name
        assert b"null" in sslib.ss_last_error_string(), name


def test_python_pcm_argument_rules(sslib):
    """int16 with pcm_scale is the one accepted pair; every rule below is raised before a handle is made (no device here)."""
    import speechsauce_amd as ss

    p1, p2, p3 = np.zeros(640, np.int16), np.zeros((2, 640), np.int16), np.zeros((2, 2, 640), np.int16)
    f1, f2 = np.zeros(640, np.float32), np.zeros((2, 640), np.float32)
    lens = ([320, 320],)
    # (function, arguments behind the signal, int16 input, float input, input of a wrong number of dimensions)
    calls = [(ss.kaldi_fbank, (), p2, f2, p3), (ss.kaldi_mfcc, (), p1, f1, p3), (ss.kaldi_fbank_packed, lens, p1, f1, p2),
             (ss.kaldi_mfcc_packed, lens, p1, f1, p2), (ss.whisper_log_mel, (), p2, f2, p3), (ss.whisper_log_mel_packed, lens, p1, f1, p2)]
    for fn, extra, pcm, flt, wrong in calls:
        with pytest.raises(TypeError):
            fn(flt, *extra, pcm_scale=2.0 ** -15)  # floats are not PCM
        with pytest.raises(TypeError):
            fn(pcm, *extra)  # int16 without pcm_scale: the dtype rule of the float form
        for other in (np.int32, np.int8, np.uint16, np.int64):
            with pytest.raises(TypeError):
                fn(pcm.astype(other), *extra, pcm_scale=2.0 ** -15)
        with pytest.raises(ValueError):
            fn(wrong, *extra, pcm_scale=2.0 ** -15)  # the number of dimensions
        for bad in (1 / 32767, 3.0, 0, -0.5, 2.0 ** 70, 2.0 ** -65, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                fn(pcm, *extra, pcm_scale=bad)
    for fn in (ss.kaldi_fbank_list, ss.kaldi_mfcc_list, ss.whisper_log_mel_list):
        with pytest.raises(TypeError):
            fn([f1, f1], pcm_scale=1.0)
        with pytest.raises(TypeError):
            fn([p1, p1])
        with pytest.raises(TypeError):
            fn([p1, p1.astype(np.int32)], pcm_scale=1.0)
        with pytest.raises(ValueError):
            fn([p1, p2], pcm_scale=1.0)
        with pytest.raises(ValueError):
            fn([p1], pcm_scale=3.0)


def test_what_the_float_front_rejected_is_still_rejected():
    import inspect

    import speechsauce_amd as ss

    x, p = np.zeros(4000, np.float32), np.zeros(4000, np.int16)
    with pytest.raises(TypeError):
        ss.kaldi_fbank(x.astype(np.float64))
    for sig, kw in ((x, {}), (p, dict(pcm_scale=1.0))):
        with pytest.raises(TypeError):
            ss.kaldi_fbank(sig, no_such_argument=1, **kw)
        with pytest.raises(TypeError):
            ss.whisper_log_mel(sig, no_such_argument=1, **kw)
        for out_of_scope in (dict(dither=1.0), dict(snip_edges=False), dict(vtln_warp=1.1)):
            with pytest.raises(ValueError):
                ss.kaldi_fbank(sig, **out_of_scope, **kw)
            with pytest.raises(ValueError):
                ss.kaldi_mfcc_packed(sig, [4000], **out_of_scope, **kw)
    for fn in (ss.kaldi_fbank, ss.kaldi_mfcc, ss.kaldi_fbank_packed, ss.kaldi_mfcc_packed, ss.kaldi_fbank_list, ss.kaldi_mfcc_list,
               ss.whisper_log_mel, ss.whisper_log_mel_packed, ss.whisper_log_mel_list):
        par = inspect.signature(fn).parameters["pcm_scale"]
        assert par.default is None and par.kind is inspect.Parameter.KEYWORD_ONLY, fn.__name__
    # the scale is an argument of the call, not of the handle: the handle cache key does not hold it
    assert "pcm_scale" not in inspect.signature(ss._kaldi_cfg).parameters
    assert list(inspect.signature(ss._get_whisper_config).parameters) == ["n_mels", "device"]
