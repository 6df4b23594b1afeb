"""float64 statement of ``air_ir_bank_convolve`` (include/air_hip.h), for the tests only: row b of a batch is
oracle/channel.py on that row's first L_b samples alone, against the response it drew cut to its own tap count, followed by
zeros; a negative index copies the row."""
import numpy as np

from oracle import channel as o_channel


def bank_oracle(x, lengths, irs, taps, idx, normalize=True):
    """x (B, Lcap) float or int16 (s / 32768); lengths, idx (B,); irs (n_ir, Hmax); taps (n_ir,) -> float64 (B, Lcap)."""
    x = np.asarray(x)
    x = x.astype(np.float64) / 32768.0 if x.dtype == np.int16 else x.astype(np.float64)
    out = np.zeros(x.shape, dtype=np.float64)
    for b, n in enumerate(lengths):
        i = int(idx[b])
        if i < 0:
            out[b, :n] = x[b, :n]
        else:
            h = np.asarray(irs[i], dtype=np.float64)[: int(taps[i])]
            out[b, :n] = o_channel.ir_convolve(x[b:b + 1, :n], h[None], [0], normalize)[0]
    return out


def row_bound(want_row, taps):
    """The bound tests/test_augment.py::test_fir_kernel_vs_oracle holds both existing forms to, per row."""
    return 2e-6 * np.abs(want_row).max() * max(1.0, np.sqrt(taps) / 8)
