"""MI355X-native TT/QTT core-arithmetic backend for TensorTrainNumerics.jl's hot path.

Host-side mirror of the reference interface (tt.py), input generators (constructors.py),
device-resident batched handles (device.py), core gradients (grad.py), the fixed-rank manifold (manifold.py), TT operator algebra (opalg.py), the multi-dimensional QTT layer (qttnd.py) and the ctypes binding of the C ABI (_lib.py).
The arithmetic lives in csrc/*.h (the kernels, and the host API in csrc/ttn_host_*.h), built through csrc/ttn_api.hip and
csrc/ttn_wg512.hip -> libttn_hip.so (hand-written HIP, gfx950).
"""
from . import _lib, constructors, cross, device, grad, manifold, opalg, pipeline, qtt, qttnd, shard, solvers, tdvp, tt
from ._lib import TTNError, build, ensure_init, finalize
from .constructors import (Delta, Delta_DN, Delta_ND, Delta_NN, H_mu, H_munu, Nabla, fourier_qtto, function_to_qtt, function_to_qtt_uniform, function_to_tensor, heisenberg_xyz_tto, id_tto, ising_tto, portable_randn,
                           qtt_basis_vector, qtt_cos, qtt_exp, qtt_polynom, qtt_sin, qtt_to_function, qtt_to_vector, qtto_constant_prolongation,
                           qtto_linear_prolongation, qtto_prolongation, pauli_matrix, pauli_pair_sum_tto, pauli_sum_tto, rand_tt, reverse_qtt_bits, shift,
                           toeplitz_to_qtto, xxx_tto, xxz_tto, xy_tto, zeros_tt, zeros_tto)
from .cross import DMRG, Greedy, MaxVol, MaxVolPivot, RandomPivot, sample_uniforms, tt_cross, tt_cross_batch, tt_integrate, tt_integrate_batch
from .device import DeviceRectTTO, DeviceTT, DeviceTTO, StreamTimer
from .grad import apply_pullback, apply_rrule, cores_axpby, cores_dot, dot_pullback, dot_rrule, rayleigh_gradient, rayleigh_value_and_grad
from .grad import expect_value_and_grad, sandwich_pullback, sandwich_rrule
from .manifold import TTManifold, TTPoint, fit_fixed_rank, rayleigh_descent, tangent_project, ttvector_manifold
from .opalg import (concatenate, kron, operator_strides, outer_product, qtto_to_matrix, tto_add, tto_compress_, tto_decomp, tto_inner, tto_mul,
                    tto_scale, tto_sub, tto_to_tensor, tto_to_ttv, ttv_to_diag_tto, ttv_to_tto)
from .solvers import (als_eigsolve, als_gen_eigsolv, crank_nicholson_method, dmrg_eigsolve, euler_method, implicit_euler_method, krylov_linsolve,
                      lowest_states, mals_eigsolve, rk4_method)
from .qttnd import (QTToperator, QTTvector, check_compat, dim_sites, entanglemententropy, function_to_qttv, grid_strides, marginal, moments, qtt_laplacian,
                    qttv_sample, qttv_to_array, reduced_meta, slice_dim)
from .qtt import bubble_sort_swaps, hadamard_ttm, reorder, reorder_op, reorder_perm, to_qtt, to_ttv, ttv_decomp
from .tt import (TToperator, TTvector, _tt_bond_truncate_, add, add_, apply, apply_compress, apply_rect, braket, contract_sites, correlation_matrix, div, dot, energy,
                 euclidean_distance, expect, hadamard, increase_ranks, norm, orthogonalize, r_and_d_to_rks, rayleigh, sandwich, scale, site_expect, sub, tt_compress_, tt_sample, tt_up_rks,
                 ttv_to_tensor, zcorrelation_matrix, zsite_expect)

__all__ = [n for n in dir() if not n.startswith("__")]
