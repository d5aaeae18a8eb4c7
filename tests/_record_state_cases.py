"""Every entry point of the C ABI, classed by what it does to a level that steps by records (ludwig_hip.hip, "Record step"), and the
case of tests/test_gpu_record_state.py that makes it the first call after record steps.

  reader   reads f / vel / rho of a level: it has to bring back what only a record holds (LW_ENSURE_POPULATIONS, LW_ENSURE_RHO)
  writer   writes them or hands out a pointer to them: before_external_write, and no record stands for them afterwards
  ruler    changes whether the level may step by records (the rule's inputs, a ban, a hold)
  neutral  neither: create / destroy / download of a set's own buffers, information, communicators
  uncovered  a reader, writer or ruler that no case reaches; tests/test_record_state_host.py allows three

A case is "test function" or "test function[parameter]" (or a tuple of such), the parameter being one of the function's PARAMETERS in
tests/test_gpu_record_state.py. An entry point that is added to the header fails tests/test_record_state_host.py until it is classed
here and, unless neutral, given a case."""

READER, WRITER, RULER, NEUTRAL, UNCOVERED = "reader", "writer", "ruler", "neutral", "uncovered"


def _r(case):
    return (READER, case)


def _n(why=""):
    return (NEUTRAL, None, why)


FIRST = "test_first_reader[%s]"
BATCH = "test_observed_batch[%s]"

ENTRY_POINTS = {
    # the library and its levels
    "ludwig_abi_version": _n(), "ludwig_last_error": _n(), "ludwig_device_count": _n(),
    "ludwig_level_create": _n(), "ludwig_level_destroy": _n(), "ludwig_level_info": _n(), "ludwig_level_block_order": _n(),
    "ludwig_level_field_layout": _n(), "ludwig_sync": _n(), "ludwig_stream_create": _n(), "ludwig_stream_destroy": _n(),
    "ludwig_record_step_rule": _n("a pure function of its arguments"), "ludwig_level_record_steps": _n(),
    "ludwig_level_set_stream": _n("changes where later work is queued, not what the arrays hold; it does not wait for the old stream"),
    "ludwig_level_add_post_collision_readers": _n("only a level with f_post_collision takes it, and such a level never steps by records"),
    "ludwig_save_old": _n("returns at once on a level without temporal storage, and a level with it never steps by records"),
    "ludwig_bouzidi_correction": _n("returns at once on a level without Bouzidi cells, and a level with them never steps by records"),
    # the state arrays
    "ludwig_level_download": _r(FIRST % "download_f"),
    # an upload of obstacle / sponge / wall_dist is a ruler as well
    "ludwig_level_upload": (WRITER, ("test_writer[upload_f]", "test_geometry_upload_changes_the_path_and_back[obstacle]")),
    "ludwig_level_field_ptr": (WRITER, "test_writer[field_ptr]"),
    "ludwig_init_equilibrium": (WRITER, "test_writer[init_equilibrium]"),
    "ludwig_level_init_from_source": (WRITER, "test_writer[init_from_source]"),
    "ludwig_level_set_rho_store": (WRITER, "test_writer[rho_store]"),
    "ludwig_halo_unpack": (WRITER, "test_writer[halo_unpack]"),
    "ludwig_halo_pack": _r(FIRST % "halo_pack"),
    # stepping
    "ludwig_step": (RULER, "test_a_level_that_becomes_a_parent_is_banned[python]"),
    "ludwig_stream_collide": (RULER, "test_both_step_entry_points_step_by_records"),
    "ludwig_execute_timestep_batch": (RULER, "test_a_level_that_becomes_a_parent_is_banned[native]"),
    "ludwig_execute_timestep_batch_observed": (RULER, BATCH % "probes-native"),
    "ludwig_execute_timestep_batch_probes": (RULER, BATCH % "probes-old_entry"),
    "ludwig_execute_timestep_batch_sampled": (RULER, BATCH % "surface_stats-old_entry"),
    "ludwig_execute_timestep_batch_loads": (RULER, BATCH % "force_series-old_entry"),
    "ludwig_execute_timestep_batch_tracers": (RULER, BATCH % "tracers-old_entry"),
    "ludwig_level_set_order": (RULER, "test_seeded_walk"),
    # readers on the level
    "ludwig_map_surface_stresses": _r(FIRST % "surface_stress_map"),
    "ludwig_level_rho_min": _r(FIRST % "rho_min"),
    "ludwig_level_stats_reset": _n(), "ludwig_level_stats_accumulate": _r(FIRST % "stats"), "ludwig_level_stats_download": _n(),
    "ludwig_level_monitor": _r(FIRST % "monitor"),
    "ludwig_level_gradient_fields_compute": _r(FIRST % "gradient_vel"), "ludwig_level_gradient_fields_download": _n(),
    "ludwig_level_subgrid_fields_compute": _r(FIRST % "subgrid_fields"), "ludwig_level_subgrid_fields_download": _n(),
    "ludwig_level_subgrid_stats_reset": _n(), "ludwig_level_subgrid_stats_accumulate": _r(FIRST % "subgrid_stats"),
    "ludwig_level_subgrid_stats_download": _n(),
    "ludwig_level_isosurface_extract": _r(FIRST % "iso_density"), "ludwig_level_isosurface_download": _n(),
    "ludwig_level_wall_census": (UNCOVERED, None, "it reads the blocks with a near-wall cell only; a level with one does not step by records, "
                                 "and the upload that makes one brings the arrays back itself. test_first_reader[wall_census] calls it, but "
                                 "its output on a plain level is the empty record whatever the flow is"),
    # observer sets
    "ludwig_probes_create": _n(), "ludwig_probes_destroy": _n(), "ludwig_probes_sample": _r(FIRST % "probes"), "ludwig_probes_download": _n(),
    "ludwig_surface_stats_create": _n(), "ludwig_surface_stats_destroy": _n(), "ludwig_surface_stats_reset": _n(),
    "ludwig_surface_stats_accumulate": _r(FIRST % "surface_stats"), "ludwig_surface_stats_download": _n(),
    "ludwig_slices_create": _n(), "ludwig_slices_destroy": _n(), "ludwig_slices_sample": _r(FIRST % "slices"), "ludwig_slices_download": _n(),
    "ludwig_streamlines_create": _n(), "ludwig_streamlines_destroy": _n(), "ludwig_streamlines_trace": _r(FIRST % "streamlines"),
    "ludwig_streamlines_download": _n(),
    "ludwig_render_create": _n(), "ludwig_render_destroy": _n(), "ludwig_render_image": _r(FIRST % "render"), "ludwig_render_download": _n(),
    "ludwig_tracers_create": _r(FIRST % "tracers"), "ludwig_tracers_destroy": _n(), "ludwig_tracers_advance": _r(FIRST % "tracers"),
    "ludwig_tracers_snapshot": _r(FIRST % "tracers"), "ludwig_tracers_download": _n(),
    "ludwig_wall_surface_create": _n(), "ludwig_wall_surface_destroy": _n(), "ludwig_wall_surface_compute": _r(FIRST % "wall_surface"),
    "ludwig_wall_surface_download": _n(),
    "ludwig_force_series_create": _n(), "ludwig_force_series_destroy": _n(), "ludwig_force_series_sample": _r(FIRST % "force_series"),
    "ludwig_force_series_download": _n(),
    "ludwig_flux_planes_create": _n(), "ludwig_flux_planes_destroy": _n(), "ludwig_flux_planes_sample": _r(FIRST % "flux_planes"),
    "ludwig_flux_planes_download": _n(),
    "ludwig_modes_create": _n(), "ludwig_modes_destroy": _n(), "ludwig_modes_reset": _n(), "ludwig_modes_accumulate": _r(FIRST % "modes"),
    "ludwig_modes_download": _n(),
    "ludwig_flow_source_create": _n("from host arrays"), "ludwig_flow_source_destroy": _n(),
    "ludwig_flow_source_from_levels": _r(FIRST % "warm_start"),
    # communicators and halo plans
    "ludwig_comm_unique_id": _n(), "ludwig_comm_create": _n(), "ludwig_comm_destroy": _n(), "ludwig_comm_allreduce_f32": _n(),
    "ludwig_halo_plan_create": (RULER, "test_halo_plan_made_mid_run"),
    "ludwig_halo_plan_pack": _r("test_halo_plan_made_mid_run"),
    "ludwig_halo_plan_unpack": (WRITER, "test_halo_plan_made_mid_run"),
    "ludwig_halo_plan_destroy": _n(), "ludwig_halo_plan_buffers": _n(), "ludwig_halo_plan_timing": _n(), "ludwig_halo_plan_in_stream": _n(),
    "ludwig_halo_plan_exchange_ms": _n(), "ludwig_halo_wait": _n("waits for an exchange; the exchange is what reads and writes"),
    "ludwig_halo_exchange": (UNCOVERED, None, "pack, send, receive and unpack through a plan, whose making has banned the record step already; "
                             "its two halves are covered as ludwig_halo_plan_pack / _unpack, the whole needs peers (real multi-rank runs)"),
    "ludwig_step_distributed": (UNCOVERED, None, "a step through a halo plan, whose making has banned the record step already; needs peers"),
}

# the test functions a case may name
CASE_FUNCTIONS = ("test_first_reader", "test_both_step_entry_points_step_by_records", "test_writer",
                  "test_geometry_upload_changes_the_path_and_back", "test_a_level_that_becomes_a_parent_is_banned",
                  "test_halo_plan_made_mid_run", "test_observed_batch", "test_seeded_walk")
MAX_UNCOVERED = 3
