"""krylov_robustness_amd -- MI355X-native trace(f(A)) evaluator.

Drop-in for the Krylov trace / matrix-function hot path of
COMPiLELab/krylov_robustness (trace_exp, mc_trace, trace_fun_update,
fun_update, fun_and_grad_krylov_{exp,fun}).  The compute lives
in libkrylov_hip.so (HIP kernels for gfx950 + C++ host driver, C ABI in
include/krylov_trace.h); this package is the Python mirror of the reference
interface used by tests and bench.py.
"""
from ._lib import KrylovError, KrylovLibraryError, FUN_CODES, LIB_PATH
from .core import (Context, DeviceMatrix, DiagEstimate, EntryEstimate, default_context, device_count, diag_fun,
                   entries_fun, expmv,
                   eigs_leading, eigs_topk, natural_connectivity_topk, frechet_entries, function_multiple_entries, hessianfcn, hessianfcn_exp,
                   hessianfcn_fun, householder_qr,
                   fun_and_grad_krylov_exp, fun_and_grad_krylov_fun, fun_update, lanczos_fmv, lanczos_fmv_auto,
                   mc_trace, normest, slq_collect, slq_plan, slq_quadforms, slq_quadforms_auto, slq_submit, slq_trace,
                   slq_trace_auto, trace_exp,
                   trace_fun_update)
from .greedy import (compute_centrality, default_greedy_tol, edge2low_rank, find_top_edges,
                     find_top_edges_fun, find_top_edges_miobi, find_top_missing_edges, find_top_nodes_miobi,
                     greedy_krylov, krylov_miobi, krylov_miobi_sharded, miobi_break, miobi_break_node, miobi_loop,
                     miobi_make, nodes_score_topk, pairs_score_topk, select_extreme, trace_fun_update_pairs,
                     krylov_break_node, trace_fun_update_nodes, diag_fun_bracket, find_top_nodes_fun, lambda_upper,
                     entries_fun_bracket, find_top_edges_bracket)
from . import datasets, matv73
from .dist import mc_trace_sharded, trace_exp_sharded
from .datasets import load_problem, load_unweighted, prepare_unweighted, prepare_weighted

__all__ = [
    "KrylovError", "KrylovLibraryError", "FUN_CODES", "LIB_PATH", "Context", "DeviceMatrix",
    "default_context", "device_count", "slq_plan", "slq_quadforms", "slq_submit", "slq_collect", "slq_trace", "slq_quadforms_auto",
    "slq_trace_auto", "normest", "diag_fun", "DiagEstimate", "entries_fun", "EntryEstimate", "find_top_edges_fun",
    "trace_fun_update", "fun_update", "fun_and_grad_krylov_exp", "fun_and_grad_krylov_fun",
    "mc_trace", "trace_exp", "expmv", "lanczos_fmv", "lanczos_fmv_auto", "trace_fun_update_pairs", "krylov_miobi",
    "greedy_krylov", "find_top_edges", "find_top_missing_edges", "compute_centrality",
    "default_greedy_tol", "krylov_miobi_sharded", "miobi_loop", "select_extreme", "function_multiple_entries", "householder_qr", "frechet_entries",
    "hessianfcn", "hessianfcn_exp", "hessianfcn_fun", "eigs_leading", "eigs_topk",
    "natural_connectivity_topk", "datasets", "matv73",
    "load_problem", "load_unweighted", "prepare_unweighted", "prepare_weighted",
    "mc_trace_sharded", "trace_exp_sharded", "edge2low_rank", "pairs_score_topk", "miobi_break", "miobi_make",
    "find_top_edges_miobi", "miobi_break_node", "nodes_score_topk", "find_top_nodes_miobi",
    "trace_fun_update_nodes", "krylov_break_node", "diag_fun_bracket", "find_top_nodes_fun", "lambda_upper",
    "entries_fun_bracket", "find_top_edges_bracket",
]
