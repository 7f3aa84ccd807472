"""Device ops: GF-GEMM, Gauss-Jordan inverse, coding matrices, synthetic data, scrub, correct, parity update, batched repair, checked repair."""
from .checked import BatchCheckedRepairPlan, CheckedRepairPlan
from .correct import BatchCorrectPlan, BatchCorrectReport, CorrectPlan, CorrectReport
from .gemm import Gemm16Plan, GemmPlan, build_desc, desc_layout, gf_gemm, pad_m, perm_tables_from_coeff, tile_for
from .inverse import PatternDecoder, decode_system16_into_plan, decode_system_into_plan, gf_invert, invert_into_plan
from .matrix import decode_matrix, encoding_matrix, gen_matrix_device, generator
from .random import fill_random_
from .repair import BatchRepairPlan
from .rows import PickPart, StripeBatch, as_rows, batch_part, check_parts, stripe_part, stripe_rows
from .scrub import BatchScrubPlan, BatchScrubReport, ScrubPlan, ScrubReport
from .update import BatchUpdatePlan, UpdatePlan

__all__ = [
    "GemmPlan", "Gemm16Plan", "build_desc", "desc_layout", "gf_gemm", "pad_m", "tile_for", "perm_tables_from_coeff",
    "PatternDecoder", "gf_invert", "invert_into_plan", "decode_system_into_plan", "decode_system16_into_plan", "decode_matrix", "encoding_matrix",
    "gen_matrix_device", "generator",
    "fill_random_",
    "BatchScrubPlan", "BatchScrubReport", "ScrubPlan", "ScrubReport",
    "BatchCorrectPlan", "BatchCorrectReport", "CorrectPlan", "CorrectReport",
    "BatchUpdatePlan", "UpdatePlan",
    "BatchRepairPlan",
    "BatchCheckedRepairPlan", "CheckedRepairPlan",
    "PickPart", "StripeBatch", "as_rows", "batch_part", "check_parts", "stripe_part", "stripe_rows",
]
