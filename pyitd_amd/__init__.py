"""pyitd_amd — MI355X (gfx950) engine for the ITD hot path of falseywinchnet/PyITD.

    from pyitd_amd import ITD, itd_baseline_extract, detect_peaks
    rows = ITD().itd(x, max_iteration=7)

Only the data-parallel path  itd(x, n) -> rotations, baseline  lives here: hand-written HIP kernels
behind a C ABI (include/pyitd_hip.h), and this host-side mirror of the reference's call surface.
"""
from . import _lib
from ._lib import ITDError, build
from .batch import instantaneous_batch, single_waves, tfe_spectrum, wave_filter, wave_histogram, Spectrum, WaveHistogram, Waves
from .engine import Engine
from .streaming import InstantaneousStream, SpectrumStream, StreamInstant, StreamSpectrum, blockwise_instantaneous
from .streaming import StreamHistogram, WaveHistogramStream, blockwise_wave_histogram
from .streaming import StreamWaves, WaveTableStream, blockwise_single_waves
from .batch import wave_filter_bounds
from .streaming import WaveBoundsStream
from .itd import (ITD, baseline_knot_estimation, detect_knots, detect_peaks, find_extrema, generate_sine_wave, instantaneous, isin, itd,
                  itd_baseline_extract, itd_baseline_extract_cubic, itd_baseline_extract_fast, itd_baseline_extract_iq, itd_batch, itd_levels,
                  itd_sine_wrapper, matlab_detect_peaks, release_engines)

from .fourier import (fourier_mode_decomposition_any, fourier_mode_decomposition_valid, itd_fourier_decomposition,
                      itd_fourier_decomposition_batch, itd_fourier_decomposition_lean)
from .spline import (crossways_itd_baseline_extract, itd_baseline_extract_modified, itd_baseline_extract_rows,
                     itd_baseline_extract_spline, mad, retrieve_statistical_image_component, totalextract2d)

__all__ = ["itd_baseline_extract_modified", "itd_baseline_extract_spline", "itd_baseline_extract_rows", "mad",
           "crossways_itd_baseline_extract", "retrieve_statistical_image_component", "totalextract2d", "ITD", "ITDError", "Engine", "build", "itd", "itd_levels", "itd_batch", "itd_baseline_extract", "detect_peaks",
           "matlab_detect_peaks", "detect_knots", "baseline_knot_estimation", "isin", "find_extrema", "generate_sine_wave",
           "itd_baseline_extract_fast", "itd_baseline_extract_cubic", "itd_baseline_extract_iq", "itd_sine_wrapper", "release_engines", "instantaneous", "instantaneous_batch", "single_waves", "wave_filter", "Waves", "tfe_spectrum", "Spectrum", "wave_histogram", "WaveHistogram", "SpectrumStream", "StreamSpectrum",
           "InstantaneousStream", "StreamInstant", "blockwise_instantaneous",
           "WaveHistogramStream", "StreamHistogram", "blockwise_wave_histogram",
           "WaveTableStream", "StreamWaves", "blockwise_single_waves",
           "wave_filter_bounds", "WaveBoundsStream",
           "fourier_mode_decomposition_any", "fourier_mode_decomposition_valid", "itd_fourier_decomposition",
           "itd_fourier_decomposition_lean", "itd_fourier_decomposition_batch"]
