"""Correlated noise by global Fourier filtering on the GPU (mirror of
pysteps/noise/fftgenerators.py:330-439, ``generate_noise_2d_fft_filter``).

The white noise is drawn from the caller's ``numpy.random.RandomState`` exactly as the reference
draws it (``randstate.randn(m, n)``: the random stream is part of the reference's result and of its
reproducibility contract, pysteps/nowcasts/steps.py:885-898); what runs on the device is everything
after that - forward transform, multiplication by the filter (inside the column pass of the inverse
transform), inverse transform, standardisation to zero mean and unit variance (csrc/cascade.hip
``psh_noise_filter_dev``).  Filters of the half-spectrum form in the spatial domain on power-of-two
grids take this path; ``use_full_fft`` filters, the spectral domain and other shapes run the
reference's own expression with the HIP FFT method object / numpy.

The filter array is uploaded once and kept on the device while the filter dictionary's array lives.

The localised generators of the same reference module - ``initialize_nonparam_2d_ssft_filter``,
``initialize_nonparam_2d_nested_filter``, ``generate_noise_2d_ssft_filter`` - live in :mod:`pysteps_amd.noise.ssft`
and are re-exported here.
"""

import numpy as np

from .. import _lib
from .._reference import lookup
from ..cascade.decomposition import _device_weights
from ..device import DeviceArray
from ..utils import fft as hip_fft
# the short-space Fourier (ssft / nested) initialisers and their generator: noise/ssft.py
from .ssft import (generate_noise_2d_ssft_filter, generate_noise_table,  # noqa: F401
                   initialize_nonparam_2d_nested_filter, initialize_nonparam_2d_ssft_filter)


def generate_noise_2d_fft_filter(F, randstate=None, seed=None, fft_method=None, domain="spatial"):
    """Produces a field of correlated noise using global Fourier filtering (parameters and return
    value as documented for the reference, fftgenerators.py:333-364)."""
    if domain not in ["spatial", "spectral"]:
        raise ValueError(
            "invalid value %s for the 'domain' argument: must be 'spatial' or 'spectral'" % str(domain)
        )
    input_shape = tuple(F["input_shape"])
    use_full_fft = F["use_full_fft"]
    field = F["field"]
    if len(field.shape) != 2:
        raise ValueError("field is not two-dimensional array")
    if np.any(~np.isfinite(field)):
        raise ValueError(
            "field contains non-finite values, this typically happens when the input\n"
            + "precipitation field provided to pysteps contains (mostly)zero values.\n"
            + "To prevent this error please call pysteps.utils.check_norain first,\n"
            + "using the same win_fun as used in this method (tukey by default)\n"
            + "and then only call this method if that check fails."
        )
    if randstate is None:
        randstate = np.random
    if seed is not None:
        randstate.seed(seed)

    if domain != "spatial" or use_full_fft or not hip_fft.supported_shape(input_shape):
        # the reference's own generator (fftgenerators.py:398-437) with the HIP transforms where they apply
        ref = lookup("noise.fftgenerators", "generate_noise_2d_fft_filter", generate_noise_2d_fft_filter)
        if ref is None:
            raise NotImplementedError("pysteps_amd generate_noise_2d_fft_filter: spatial domain, half-spectrum filters and "
                                      "power-of-two grids run on the HIP path; pysteps is not importable for the rest")
        fft = fft_method
        if (fft is None or isinstance(fft, str)) and hip_fft.supported_shape(input_shape):
            fft = hip_fft.get_hip(input_shape)
        return ref(F, randstate=randstate, seed=None, fft_method=fft, domain=domain)

    m, n = input_shape
    if tuple(field.shape) != (m, n // 2 + 1):  # the reference fails broadcasting fN *= F (:420)
        raise ValueError("operands could not be broadcast together with shapes (%d,%d) %s" % (m, n // 2 + 1, tuple(field.shape)))
    white = randstate.randn(m, n)  # fftgenerators.py:400
    d_white = DeviceArray.from_host(white)
    d_filter = _device_weights(field)
    out = DeviceArray((m, n), np.float64)
    _lib.check(_lib.lib().psh_noise_filter_dev(d_white.ptr, d_filter.ptr, m, n, out.ptr), "psh_noise_filter_dev")
    return out.to_host()
