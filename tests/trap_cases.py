"""Offline TRAP-DCT over its shape space: the cases, inputs and references tests/test_trapdct_shapes.py (GPU) and
tests/test_trapdct_shapes_cpu.py (no GPU) share.

The operation (src/fea/fea_trap.cc:53-127 of the reference): out[t][b * ndct + k] = sum_j G[k][j] * logmel[clamp(t - half + j, 0, T - 1)][b],
half = (traplen - 1) / 2, G = config_table(cfg, "trap") [ndct][traplen] (mean removal, Hamming and REDFT10 folded, coefficient 0 dropped).

The inputs are cut from the bundled recordings CS0 and CS3: on synthetic speech a single fp32 chain over 255 taps stays inside the parity
bound (5.9e-5), on the recordings it does not (1.9e-4), and the float32 rounding of the log-mel rows alone costs up to 6.7e-5 on
synth_utt at 50 bands - more than the half of the bound the conditions below leave to the inputs."""
import numpy as np

from tests.util import C2, sig

WINDOW, SHIFT = 400, 160   # C2: 25 ms / 10 ms at 16 kHz
TOL = 1e-4                 # the project's parity bound (tests/test_gpu_parity.py)

# (kernel path as config_table(cfg, "trap_path")[:3] gives it: split16, NRB, NSM), -fb_definition, traplen, ndct, what the case covers
SPLIT16, M1_26, M2_26, M1_64, M2_64 = (1, 0, 0), (0, 1, 26), (0, 2, 26), (0, 1, 64), (0, 2, 64)
CASES = [
    (SPLIT16, "23filters", 101, 16),      # C5's shape
    (SPLIT16, "23filters", 113, 16),      # last context of the split kernel; tile origin = first tap
    (SPLIT16, "24filters", 113, 16),      # NF = 6 exactly full
    (SPLIT16, "23filters", 3, 2),         # half 1; D = 46, scalar stores
    (SPLIT16, "23filters", 51, 15),       # ndct one below the vector store
    (SPLIT16, "1-5/5filters", 31, 16),    # fewer bands than waves
    (SPLIT16, "1-8/8filters", 31, 16),    # one band per wave
    (M1_26, "26filters", 103, 16),        # last short context; vector store
    (M1_26, "26filters", 31, 5),          # scalar store
    (M1_26, "25filters", 31, 16),         # odd B: B | 1 == B
    (M2_26, "23filters", 101, 17),        # ndct alone takes it off the split kernel
    (M2_26, "26filters", 33, 17),
    (M2_26, "26filters", 51, 20),
    (M2_26, "26filters", 51, 32),         # ndct maximum
    (M1_64, "23filters", 115, 16),        # first context past the split kernel
    (M1_64, "26filters", 105, 16),        # 27 tap groups
    (M1_64, "23filters", 201, 16),
    (M1_64, "23filters", 253, 16),        # three padded taps
    (M1_64, "23filters", 255, 16),        # largest context
    (M2_64, "50filters", 255, 32),        # largest of everything; D = 1600; 67 284 bytes of LDS
    (M2_64, "1-51/51filters", 245, 17),   # 65 692 bytes of LDS, the first past 64 KiB: the launch raises the kernel's limit
]
SMALLEST, LARGEST = CASES[3], CASES[19]


def case_id(case):
    return "%s_%d_%d" % (case[1].replace("filters", "").replace("/", "of"), case[2], case[3])


def n_bands(bank):
    return int(bank.replace("filters", "").split("/")[-1])


def trap_cfg(case):
    return C2 + ["-fb_definition", case[1], "-fea_kind", "trapdct,%d,%d" % (case[2], case[3])]


def logspec_cfg(case):
    """The same options with the log-mel rows themselves as the feature: what the TRAP kernel reads."""
    return C2 + ["-fb_definition", case[1], "-fea_kind", "logspec"]


def frame_counts(traplen):
    """half + 1 (the fewest the plan takes: both clamps fall in one tile), the chunk of trapdct_mfma_kernel and its neighbours, one
    frameless utterance in the middle, the chunk of trapdct_split16_kernel and its neighbours, 200; none below half + 1."""
    half = (traplen - 1) // 2
    low = [half + 1] + [c for c in (63, 64, 65) if c > half + 1]
    high = [c for c in (127, 128, 129, 200) if c > half + 1]
    assert sum(low + high) < 900
    return low + [0] + high


def utterances(case):
    """One list for one Engine.extract call: the frame counts above, cut in turn from CS0 and CS3 at offsets of their own, each with
    half a hop of samples that complete no frame; the frameless one is 300 samples."""
    rec = [sig("CS0"), sig("CS3")]
    out = []
    for i, f in enumerate(frame_counts(case[2])):
        n = WINDOW + (f - 1) * SHIFT + SHIFT // 2 if f else 300
        x = rec[i % 2]
        at = (2500 + 11000 * i) % (x.size - n)   # (moved until every case met test_the_inputs_leave_the_kernel_half_of_the_bound)
        out.append(x[at:at + n].copy())
    return out


def contract(G, L, traplen, ndct, fault=None):
    """R64[t][b * ndct + k] = sum_j G[k][j] * L[clamp(t - half + j, 0, T - 1)][b] in float64; G [ndct][traplen], L [T][B].
    `fault`: one of the ways a kernel gets this wrong (FAULTS), for the tests that show the comparator sees them."""
    G = np.asarray(G, np.float64).reshape(ndct, traplen)
    L = np.asarray(L, np.float64)
    T, B = L.shape
    if T == 0:
        return np.zeros((0, B * ndct))
    half = (traplen - 1) // 2
    j = np.arange(traplen)
    if fault == "first_tap_dropped":
        G = G.copy(); G[:, 0] = 0.0
    elif fault == "last_tap_dropped":
        G = G.copy(); G[:, -1] = 0.0
    elif fault == "padded_tap_weighted":   # tap `traplen` of the padded group takes the last real weight
        G = np.concatenate([G, G[:, -1:]], axis=1)
        j = np.arange(traplen + 1)
    idx = np.arange(T)[:, None] - half + j[None, :] + (1 if fault == "context_shifted" else 0)
    hi = T if fault == "right_clamp_at_T" else T - 1   # frame T is whatever lies behind the utterance: here the first frame again
    idx = np.clip(idx, 0, hi) % T
    if fault == "bands_swapped":
        L = L.copy(); L[:, [0, 8 % B]] = L[:, [8 % B, 0]]
    R = np.einsum("kj,tjb->tbk", G, L[idx])
    return R.reshape(T, B * ndct)


FAULTS = ("first_tap_dropped", "last_tap_dropped", "context_shifted", "right_clamp_at_T", "padded_tap_weighted", "bands_swapped")


def operation_error(K, R64):
    """max |K - R64| / max(|R64|, 1): the project's tolerance applied to the contraction alone."""
    return float((np.abs(np.asarray(K, np.float64) - R64) / np.maximum(np.abs(R64), 1.0)).max()) if R64.size else 0.0
