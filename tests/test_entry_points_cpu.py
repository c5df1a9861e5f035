"""What every entry point of the C ABI answers before psh_init (no GPU): the table below, fixed on the commit before the
entry guard (csrc/entry.h) and unchanged by it.

tests/helpers/entry_points.py loads the built library without initialising it and calls every name of _lib.SIGNATURES but
psh_init, psh_shutdown, psh_last_error and psh_version with every argument zero or NULL, each in a forked child.  The
same calls are repeated in-process after the last psh_shutdown by tests/helpers/shutdown_cycle.py (GPU)."""

import json
import os
import subprocess
import sys

from conftest import ROOT

from pysteps_amd import _lib

NOT_CALLED = ("psh_init", "psh_shutdown", "psh_last_error", "psh_version")
# the guard is the first statement
ENOTINIT = (
    "psh_anvil_diff_dev", "psh_anvil_gauss_dev", "psh_anvil_masks_dev", "psh_anvil_phi_dev", "psh_anvil_rvil_dev",
    "psh_anvil_update_dev", "psh_ar_iterate_dev", "psh_autocorr_spectral_sums_dev", "psh_autocorr_sums_dev",
    "psh_autocorr_window_prepare_dev", "psh_axpy_f64_dev", "psh_blend_db_inverse_f64_dev",
    "psh_blend_dense_rank_dev", "psh_blend_linear_dev", "psh_blend_salient_dev", "psh_blend_scale_dev",
    "psh_blob_cube_dev", "psh_blob_gather_dev", "psh_blob_peaks_dev", "psh_cascade_decompose_dev",
    "psh_cascade_decompose_levels_dev", "psh_cascade_recompose_dev", "psh_comm_allgather", "psh_comm_allreduce_f32",
    "psh_comm_broadcast", "psh_comm_init", "psh_convert_dev", "psh_count_above_dev", "psh_crps_sums_dev",
    "psh_darts_band_dev", "psh_darts_gram_dev", "psh_darts_nonfinite_dev", "psh_darts_rows_dev",
    "psh_darts_synth_dev", "psh_db_transform_dev", "psh_dense_lk_dev", "psh_dense_lk_uv_dev",
    "psh_detcat_counts_dev", "psh_detcat_pairs_dev", "psh_detcont_pairs_dev", "psh_detcont_sums_dev",
    "psh_device_info", "psh_dilated_mask_dev", "psh_ens_products_dev", "psh_event_create", "psh_event_destroy",
    "psh_event_elapsed_ms", "psh_event_record", "psh_expand_compact_c128_dev", "psh_fft_c2c2_dev",
    "psh_fft_irfft2_dev", "psh_fft_irfft2_min_dev", "psh_fft_rfft2_dev", "psh_field_min_key_dev",
    "psh_field_stats_dev", "psh_field_transform_dev", "psh_fss_sums_dev", "psh_ge_mask_dev", "psh_host_alloc",
    "psh_idw_dev", "psh_idw_host", "psh_lagprob_dev", "psh_lerp_dev", "psh_lk_band_open_dev",
    "psh_lk_band_response_dev", "psh_lk_band_select_dev", "psh_lk_band_stats_dev", "psh_lk_band_to_u8_dev",
    "psh_lk_corners_finish", "psh_lk_corners_launch_dev", "psh_lk_order_host", "psh_lk_prepare_dev",
    "psh_lk_prepare_f64_dev", "psh_lk_pyramids_dev", "psh_lk_track_pyr_dev", "psh_malloc", "psh_mask_count_dev",
    "psh_mask_row_offsets_dev", "psh_masked_moments_dev", "psh_members_disp_to_state_dev", "psh_members_pack_dev",
    "psh_members_state_to_disp_dev", "psh_memcpy_d2d", "psh_memcpy_d2h", "psh_memcpy_d2h_async", "psh_memcpy_h2d",
    "psh_memset", "psh_nan_where_dev", "psh_noise_adj_centre_dev", "psh_noise_adj_observed_dev",
    "psh_noise_adj_prepare_dev", "psh_noise_filter_dev", "psh_nonfinite_count_f64_dev", "psh_nqt_count_le_dev",
    "psh_nqt_forward_dev", "psh_nqt_inverse_dev", "psh_nqt_table_dev", "psh_outliers_local_host",
    "psh_probbins_dev", "psh_probmatch_dev", "psh_proesmans_consistency_dev", "psh_proesmans_dev",
    "psh_proesmans_gradients_dev", "psh_proesmans_next_level_dev", "psh_proesmans_pyramid_dev",
    "psh_proesmans_scale_dev", "psh_proesmans_sweep_dev", "psh_rainfarm_exp_dev", "psh_rainfarm_finish_dev",
    "psh_rainfarm_spectrum_dev", "psh_rainfarm_std_dev", "psh_rapsd_counts_dev", "psh_rapsd_fill_nan_dev",
    "psh_rapsd_full_dev", "psh_rapsd_half_dev", "psh_rapsd_nonfinite_dev", "psh_rbf_eval_dev", "psh_rng_check",
    "psh_rng_create", "psh_rng_destroy", "psh_rng_get_state", "psh_rng_randn_dev", "psh_rng_uniform_dev",
    "psh_rng_wait", "psh_semilag_dev", "psh_semilag_host", "psh_semilag_members_dev",
    "psh_semilag_members_state_dev", "psh_semilag_rows_dev", "psh_semilag_uv_dev", "psh_spectrum_level_moments_dev",
    "psh_ssft_generate_dev", "psh_ssft_local_filters_dev", "psh_ssft_merge_dev", "psh_ssft_war_counts_dev",
    "psh_steps_ar_recompose_dev", "psh_steps_incremental_mask_dev", "psh_steps_mask_dev",
    "psh_steps_mean_shift_dev", "psh_steps_phase_ar_dev", "psh_steps_spectral_ar_dev",
    "psh_steps_spectral_sums_dev", "psh_sync", "psh_vectors_finish_host", "psh_velocity_unit_dev",
    "psh_window_corrcoef_dev",
)
# an argument check stands in front of the guard, or the function is pure host code that needs no device
EINVAL = (
    "psh_cascade_decompose_stats_dev", "psh_comm_unique_id", "psh_decluster_host", "psh_lk_corners_dev",
    "psh_lk_greedy_host", "psh_lk_pyramids_band", "psh_lk_pyramids_read", "psh_lk_pyramids_shape",
    "psh_order_statistic_dev", "psh_probmatch_async_dev", "psh_probmatch_plan_create", "psh_probmatch_planned_dev",
    "psh_semilag_members_packed_dev", "psh_set_option", "psh_steps_ar_recompose_raw_dev",
    "psh_steps_mask_probmatch_dev",
)
# releasing nothing, an empty point list, questions answered on the host: fine without a device
OK = (
    "psh_comm_destroy", "psh_free", "psh_host_free", "psh_lk_pyramids_free", "psh_lk_track_dev",
    "psh_probmatch_plan_destroy", "psh_probmatch_status", "psh_proesmans_sweep_launches", "psh_semilag_window_shape",
)
# plain values, not status codes
VALUES = {"psh_comm_unique_id_bytes": 128, "psh_semilag_kernel": 1}

EXPECTED = dict(VALUES)
EXPECTED.update({name: _lib.PSH_ENOTINIT for name in ENOTINIT})
EXPECTED.update({name: _lib.PSH_EINVAL for name in EINVAL})
EXPECTED.update({name: _lib.PSH_OK for name in OK})


def test_every_entry_point_has_exactly_one_row():
    assert len(EXPECTED) == len(ENOTINIT) + len(EINVAL) + len(OK) + len(VALUES)  # no name in two rows
    assert set(EXPECTED) == set(_lib.SIGNATURES) - set(NOT_CALLED), sorted(set(EXPECTED) ^ (set(_lib.SIGNATURES) - set(NOT_CALLED)))


def test_what_every_entry_point_answers_before_psh_init():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "entry_points.py")],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    got = json.loads(run.stdout.strip().split("\n")[-1])
    assert sorted(got) == sorted(EXPECTED)
    wrong = {name: (got[name], EXPECTED[name]) for name in EXPECTED if got[name] != EXPECTED[name]}
    assert not wrong, wrong  # name -> (answered, expected); "signal N": the child crashed
