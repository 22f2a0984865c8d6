"""MI355X-native framewise speech feature engine (CtuCopy-compatible hot path)."""
from .engine import CtuError, Engine, Plan, Streams, config_dims, config_table, load_library, streams_config_check, streams_config_check_ex, streams_flags_for, streams_rows_step, streams_signal_step, streams_step, streams_vad_rows_step, streams_vad_step, wire_expand, wire_extent  # noqa: F401
