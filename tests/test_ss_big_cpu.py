"""hwss / fwss / 2fwss at FFT sizes of 2048 and 4096 points are on the accelerated path (bigss_kernel.h): without a GPU the engine gets
as far as opening the device (unsupported_reason runs before that), and what stays outside the path is still reported."""
import pytest

import ctucopy_amd
from ctucopy_amd import CtuError
from ctucopy_amd import build as cbuild
from ctucopy_amd import engine as ceng
from oracle.oracle import Oracle

B = ["-vad", "burg"]


def M(fs):
    return f"-fs {fs} -format_in raw -format_out htk -preset mfcc -preem 0.97".split()


W64 = ["-w", "64", "-s", "20"]   # 3072 samples at 48 kHz: 4096 points
FEATURE_CONFIGS = [
    M(44100) + B + ["-nr_mode", "fwss"],                                                         # 1103 samples, 2048 points
    M(44100) + B + ["-nr_mode", "2fwss"],
    M(44100) + B + ["-nr_mode", "hwss", "-fea_kind", "spec", "-nr_a", "2", "-nr_b", "1.5"],
    M(44100) + B + ["-nr_mode", "fwss", "-fea_kind", "logspec", "-fea_ncepcoefs", "20"],          # a detector of 20 coefficients
    M(44100) + B + ["-nr_mode", "fwss", "-fea_E", "on", "-fea_delta", "d_a"],
    M(44100) + B + ["-nr_mode", "fwss", "-fea_kind", "lpc", "-fea_lporder", "12", "-fb_inld", "on", "-fb_eqld", "on"],
    M(44100) + B + ["-nr_mode", "2fwss", "-fb_power", "off", "-fea_kind", "logspec", "-fea_E", "on"],
    M(48000) + W64 + B + ["-nr_mode", "fwss"],
    M(48000) + W64 + B + ["-nr_mode", "2fwss", "-nr_p", "0.9", "-nr_q", "0.95"],
]
SIGNAL_CONFIGS = [
    "-fs 44100 -format_in raw -format_out raw -preset exten -nr_mode fwss -vad burg".split(),
    "-fs 48000 -format_in raw -format_out raw -preset exten -nr_mode 2fwss -vad burg -w 64 -s 32".split(),
]
K1024 = "-fs 16000 -preset mfcc -w 40 -nr_mode fwss -vad burg".split()   # 640 samples: 1024 points, wave1k_kernel's size


def ident(c):
    return " ".join(c[c.index("-preset") + 2:]) + (" @" + c[1])


@pytest.fixture(scope="module", autouse=True)
def _built():
    cbuild.build_engine()


@pytest.mark.parametrize("cfg", FEATURE_CONFIGS + SIGNAL_CONFIGS, ids=ident)
def test_spectral_subtraction_reaches_the_device_at_2048_and_4096_points(cfg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    Oracle(cfg)   # the checker accepts the configuration
    with pytest.raises(CtuError) as ei:
        ctucopy_amd.Engine(cfg)
    assert ei.value.code == ceng.CTU_ERR_DEVICE and "no CPU fallback" in str(ei.value), str(ei.value)


def test_what_stays_outside_the_path_is_still_reported():
    base = M(44100) + B + ["-nr_mode", "fwss"]
    for cfg in (["-format_in", "raw", "-format_out", "htk"] + K1024,      # 1024 points: refused whole, features
                ["-format_in", "raw", "-format_out", "raw"] + K1024,      # and speech output
                base + ["-stat_cmvn", "s.txt"],
                base + ["-nr_when", "afterFB"],
                base + ["-vad_out_mode", "vad"],
                base + ["-vad_apply_mode", "silence"],
                base + ["-remove_dc1", "on"],
                base + ["-fea_kind", "trapdct,101,16"],
                base + ["-fea_ncepcoefs", "33", "-fea_kind", "logspec"]):  # a detector of 33 coefficients
        with pytest.raises(CtuError) as ei:
            ctucopy_amd.Engine(cfg)
        assert ei.value.code == ceng.CTU_ERR_UNSUPPORTED, (cfg, str(ei.value))
