"""CPU-only tests of where the Python wrappers live ("Where the Python wrappers live"): rfn_hip.ops keeps
every public name it had before the leaf wrappers moved into modules of their own, each moved name is the object of
its home module, and no module of the package imports ops back."""
import ast
import glob
import importlib
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "recurrent-flows-msc_amd", "rfn_hip")

# [n for n in dir(ops) if not n.startswith("_") and not isinstance(getattr(ops, n), types.ModuleType)] at the commit
# before the split (2a49aad): 160 names
PUBLIC_AT_PARENT = (
    "ACT", "BatchNormFlowFn", "CLAMP", "CLIP_MIRROR", "CLIP_REVERSE", "CONV_PRECISION", "ConvFn",
    "ConvLSTMCellFn", "ConvLSTMSeqFn", "CouplingRoute", "FinishTicket", "GAUSS_HEADS_OUTPUTS", "GaussHeadsFn",
    "GaussLogpFn", "GlowLevelFn", "GlowStepFn", "GlowStepRevFn", "I3DWeights", "INVCONV_MAX_CHANNELS",
    "INVCONV_MAX_STEPS", "InvConvWeightsFn", "KEYED_NORMAL_MAX_SLOTS", "KEYED_UNIFORM_SLOT_DEQUANT",
    "LEVEL_MIRRORED_MIN_PIXELS", "LSTMCellFn", "LSTM_CELL_KERNEL_DEFAULT", "LatentStepFn", "LinearExtrapLossFn",
    "LpipsAlexWeights", "LpipsFeatures", "MIXED_FWD", "MOL_KEYED_SLOT_COLOUR", "MOL_KEYED_SLOT_MIX", "MolNllFn",
    "NetGrads", "POPackPlan", "PackBatch", "PackPlan", "RESIZE_MAX_SIDE", "SHEET_MAX_ROWS", "STEP_NPARAM",
    "Squeeze2dFn", "StepBatchNormActFn", "StepBatchNormActPoolFn", "StepPacks", "StepParams", "TAP_MAX_COUT",
    "TailGrads", "Up2xCatFn", "WGRAD_BAND_MIN_PIXELS", "WgradOperands", "WgradPlan", "ZeroArena",
    "actnorm_invconv_bwd", "actnorm_invconv_fwd", "affine_coupling_", "bnflow_apply", "bnflow_coef", "bwd_b3",
    "channel_stats", "chart_chunk", "chart_font", "clip_gather", "clip_gather_aug", "compose_sheet",
    "conv2d_dgrad_act", "conv2d_raw", "conv2d_wgrad", "conv2d_wgrad_grouped", "conv3x3_c1_wgrad16",
    "conv3x3_fewcin", "conv3x3_smallcout", "conv_ep", "conv_epilogue_bwd", "convlstm_seq_supported",
    "coupling_po_bwd", "coupling_po_bwd_finish", "coupling_po_bwd_ok", "coupling_po_fwd", "coupling_po_ok",
    "coupling_route", "dgrad_small_ok", "fewcin_ok", "frame_quality", "frames_resize", "frechet_distance",
    "fwd_prec", "gather_affine_", "gauss_heads", "gauss_heads_check", "gauss_logp", "gauss_quality",
    "gauss_quality_check", "gauss_sample", "gemm_wgrad", "gemm_wgrad_grouped", "group_level_wgrad",
    "grouped_wgrad_budget", "grouped_wgrad_retained_bytes", "i3d_embed", "i3d_head", "i3d_inception",
    "i3d_load", "i3d_logits", "i3d_maxpool", "i3d_pack", "i3d_preprocess", "i3d_same", "i3d_sizes", "i3d_unit",
    "invconv_actnorm_rev", "invconv_weights_ok", "kernel_label", "keyed_normal", "keyed_normal_tiled_row",
    "keyed_uniform", "latent_iw", "level_mirrored_min_pixels", "linear_extrap_check", "linear_extrap_loss",
    "linear_extrap_pairs", "linear_extrap_rollout", "linext_limits", "lpips_alex", "lpips_alex_distance",
    "lpips_alex_features", "lpips_alex_load", "lpips_alex_pack", "lpips_alex_sizes", "lstm_cell",
    "lstm_cell_check", "lstm_cell_route", "lstm_cell_torch", "mol_dims", "mol_keyed_uniforms", "mol_nll",
    "mol_sample", "mol_sample_keyed", "moving_mnist_render", "moving_mnist_sync_render", "pack_weight",
    "render_chart", "resize_window", "sheet_shape", "smallmap_arith_ok", "smallmap_conv", "smallmap_conv_ok",
    "smallmap_dense", "smallmap_dense_pair", "smallmap_pack", "smallmap_supported", "squeeze2d_raw", "wgrad_b3",
    "wgrad_band_min_pixels", "wgrad_plan", "wgrad_short_rows", "zeros_conv_fwd", "zeros_conv_uses_taps",
    "zeros_conv_wgrad", "zeros_conv_wgrad_grouped")

# home module -> the public names that moved into it
HOMES = {
    "gauss_heads": ("GAUSS_HEADS_OUTPUTS", "gauss_heads_check", "GaussHeadsFn", "gauss_heads"),
    "lstm_cell": ("lstm_cell_check", "LSTM_CELL_KERNEL_DEFAULT", "lstm_cell_route", "lstm_cell_torch", "LSTMCellFn",
                  "lstm_cell"),
    "stepbn": ("StepBatchNormActFn", "StepBatchNormActPoolFn", "Up2xCatFn"),
    "bnflow": ("bnflow_coef", "BatchNormFlowFn", "bnflow_apply"),
    "mol": ("mol_dims", "MolNllFn", "mol_nll", "mol_sample", "MOL_KEYED_SLOT_MIX", "MOL_KEYED_SLOT_COLOUR",
            "mol_sample_keyed", "mol_keyed_uniforms"),
    "frame_metrics": ("frame_quality",),
    "linext": ("linext_limits", "linear_extrap_pairs", "linear_extrap_check", "LinearExtrapLossFn", "linear_extrap_loss",
               "linear_extrap_rollout", "gauss_quality_check", "gauss_quality"),
    "frames": ("moving_mnist_render", "moving_mnist_sync_render", "clip_gather", "CLIP_MIRROR", "CLIP_REVERSE",
               "clip_gather_aug", "RESIZE_MAX_SIDE", "resize_window", "frames_resize"),
    "noise": ("KEYED_NORMAL_MAX_SLOTS", "keyed_normal_tiled_row", "keyed_normal", "KEYED_UNIFORM_SLOT_DEQUANT",
              "keyed_uniform"),
    "pictures": ("SHEET_MAX_ROWS", "sheet_shape", "compose_sheet", "chart_chunk", "chart_font", "render_chart"),
}


def test_ops_keeps_every_public_name():
    from rfn_hip import ops
    assert len(set(PUBLIC_AT_PARENT)) == 160
    assert [n for n in PUBLIC_AT_PARENT if not hasattr(ops, n)] == []


def test_moved_names_are_their_home_modules_objects():
    from rfn_hip import ops
    for module, names in HOMES.items():
        home = importlib.import_module("rfn_hip." + module)
        for n in names:
            assert n in PUBLIC_AT_PARENT, n
            assert getattr(ops, n) is getattr(home, n), (module, n)
        # a function or class defined in a home module is listed above (and so re-exported and checked)
        defined = [n for n, v in vars(home).items()
                   if not n.startswith("_") and getattr(v, "__module__", None) == home.__name__]
        assert sorted(set(defined) - set(names)) == [], module


def _imports_ops(tree):
    """the places of a module's syntax tree that import rfn_hip.ops: `from . import ops`, `from .ops import ...`,
    `import rfn_hip.ops`, `from rfn_hip import ops`, `from rfn_hip.ops import ...`, or the dotted name rfn_hip.ops"""
    found = []
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom):
            module = node.module or ""
            if module in ("ops", "rfn_hip.ops") or module.endswith(".ops"):
                found.append(node.lineno)
            elif module in ("", "rfn_hip") and any(a.name == "ops" for a in node.names):
                found.append(node.lineno)
        elif isinstance(node, ast.Import):
            if any(a.name == "rfn_hip.ops" for a in node.names):
                found.append(node.lineno)
        elif isinstance(node, ast.Attribute) and node.attr == "ops":
            if isinstance(node.value, ast.Name) and node.value.id == "rfn_hip":
                found.append(node.lineno)
    return found


def test_no_module_imports_ops_back():
    assert _imports_ops(ast.parse("from . import ops")) and _imports_ops(ast.parse("def f():\n    from .ops import x"))
    assert _imports_ops(ast.parse("import rfn_hip\nrfn_hip.ops.x()")) and not _imports_ops(ast.parse("from . import lib"))
    files = sorted(glob.glob(os.path.join(PKG, "*.py")))
    assert len(files) >= 20
    for path in files:
        if os.path.basename(path) in ("ops.py", "__init__.py"):
            continue
        with open(path) as f:
            assert _imports_ops(ast.parse(f.read())) == [], path
