"""Noise generators and the noise adjustment on the HIP path (mirror of pysteps.noise.fftgenerators / .utils)."""

from .fftgenerators import (generate_noise_2d_fft_filter, generate_noise_2d_ssft_filter,  # noqa: F401
                            initialize_nonparam_2d_nested_filter, initialize_nonparam_2d_ssft_filter)
from .utils import compute_noise_stddev_adjs  # noqa: F401
