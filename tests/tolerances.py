"""The parity contract of the device path, in ONE place (tests, __graft_entry__.smoke and DESIGN.md section 2 quote it).

north_star asks 1e-3 relative on bf16 logits.  With 8-bit-mantissa MFMA operands that is below the rounding floor
(frozen weights in bf16 alone: 5.1e-3 at depth 12, oracle error budget in DESIGN.md section 2), so the bar the tests
hold is "the kernels add no error of their own":

* whole-model logits, rel-L2 against the fp32 reference / as-written oracle:  <= LOGITS_VS_MODEL x what the oracle
  evaluated with the SAME bf16 rounding points (``bf16_sim``) is away from fp32, and <= LOGITS_ABS;
* every CP / head gradient against fp32 autograd of the as-written algorithm:  <= CP_GRAD rel-L2;
* ONE block on the same (bf16-representable) inputs, device vs ``bf16_sim``:   <= BLOCK_VS_SIM rel-L2 (measured 2e-4 attention, 3e-5 MLP);
* class indices: exact wherever the fp32 top-2 margin exceeds the measured logit noise.
"""
LOGITS_ABS = 1.0e-2
LOGITS_VS_MODEL = 1.15
MODEL_FLOOR = 4.0e-3     # for tiny cases whose rounding-model error is itself near zero
CP_GRAD = 2.5e-2
BLOCK_VS_SIM = 1.0e-3
# Backward, device against its rounding model directly (tests/test_backward_contract_gpu.py): at most this many times the distance
# between the model and its own second evaluation with fp32 accumulators in another summation order -- room for the rounding ties
# that flip between two orders.  Held only for parts where that yardstick times this factor is below the model's own error against
# fp64; measured yardsticks and device figures: docs/findings/backward_contract.md section 5.
BWD_VS_MODEL_ORDER = 4.0
# CPU results against vectors recorded on one host: what goes through the host's math library (orthogonal_'s QR, an fp32
# forward) rounds its last bits by that host's kernels, 1.6e-6 apart at most between two x86 hosts (rank 64); a different
# draw order or initialiser moves entries by ~0.1.  What comes straight from the RNG is compared bitwise.
HOST_ATOL = 1.0e-5

# The kernels around the blocks (oracle/small_kernels.py): a 16-bit output may be the NEIGHBOUR of the model's rounded value only
# where the float64 value lies within the derived fp32 error term of a rounding boundary, and only this share of a tensor's
# elements may use that.  Each cap is chosen with the test inputs (tests/test_small_kernels_model.py): an fp32 restatement of the
# kernel in another summation order uses at most HALF of it on every case, on the host; never fitted to a device.  Shares per
# case: docs/findings/small_kernels_contract.md.
# Row families of tests/test_small_kernels_model.py::family_rows: 0 Gaussian, 1 offset (mean 100, spread 1e-2), 2 constant, 3 one
# outlier channel, 4 tiny, 5 all zero.  The other-order restatement's largest share over all cases and both operand types is 0.0039
# (one element of a 256-wide outlier row; Gaussian 0.0013, tiny 0.0007, constant and zero rows none), so twice that, rounded up to
# 2 %, is the cap of every family but one.  The OFFSET rows have no cap (None): there the derived term -- gamma(kappa + 2) |mu| rstd
# = 20 x 2^-24 x 100 x 100 = 1.2e-2 -- is several 16-bit steps of y (bf16 7.8e-3, fp16 9.8e-4 at 1), the restatement itself moves
# 92 % of an fp16 row off the model's value, and a cap below 1 would be fitted, not derived: the interval alone holds those rows.
# "xu_T" (T = y U and G' = dyb U of the fused LayerNorm kernels): counted over all M of one (C, rank, build) -- at M = 1 a tensor
# has 32 elements and ONE neighbour case is 3 % -- where the restatement uses at most 0.0013 (fp16; none in bf16): the same 2 %.
_FAMILY_CAPS = {0: 0.02, 1: None, 2: 0.02, 3: 0.02, 4: 0.02, 5: 0.02}
SMALL_CAPS = {"ln_y": _FAMILY_CAPS, "ln_dyb": 0.02, "head_xn16": _FAMILY_CAPS, "head_dxn": 0.02, "xu_T": 0.02}


def logits_ok(r_ref: float, r_model: float) -> bool:
    return r_ref <= LOGITS_ABS and r_ref <= LOGITS_VS_MODEL * max(r_model, MODEL_FLOOR)

# The GEMM family (oracle/gemm_model.py), per 16-bit output kind: the share of a tensor's elements that may be the NEIGHBOUR of the
# model's rounded value, taken over the elements whose derived term is below a quarter of their own 16-bit step.  Elements above
# that -- the cancelling rows (|acc| << sum |a b|: gamma(K) sum |a b| is many steps of a sum near zero), the GELU's negative tail
# (a step of h = -1e-6 is 1e-8, the pre-activation's term 1e-6), sums that happen to land near zero -- have NO cap: the interval
# alone holds them, as it does the offset LayerNorm rows above.  ONE neighbour case never breaks a cap (M = 1, N = 8: 12 %).
# Chosen as SMALL_CAPS: the fp32 other-order restatement's largest share over all host cases and both builds
# (tests/test_gemm_model.py, `python -m tests.test_gemm_model`; table in docs/findings/gemm_contract.md section 2), doubled and rounded
# up to the next of 0.5 %, 1 %, 2 %; never fitted to a device.  Measured: gelu_h 0.0030 (fp16; bf16 none) -> 1 %; dgelu 0.0010
# (fp16; bf16 0.0006) -> 0.5 %; bf16, T 0.0001 (fp16), gelu_u, gelu_dg, mulh none -> 0.5 %.
GEMM_CAPS = {"bf16": 0.005, "gelu_h": 0.01, "gelu_u": 0.005, "gelu_dg": 0.005, "dgelu": 0.005, "mulh": 0.005, "T": 0.005}

# The adapter-side kernels (oracle/adapter_model.py), per 16-bit output kind, under the same rule as GEMM_CAPS (the share is taken
# over the elements whose derived term is below a quarter of their own 16-bit step; one neighbour case never breaks a cap).
# "pack": the entries of cara_factor_prep's pack that are products of one to five fp32 numbers (Vs_*, U_fc2; the copies U_qkv,
# U_proj, U_fc1 are held bitwise), all layers of one matrix taken as one tensor.  Their derived term gamma(5) |v| = 3e-7 |v| is at most 1 / 13000 of
# a bf16 step (2^-8 |v| or more) and 1 / 1600 of an fp16 step (2^-11 |v| or more), so every element is capped and a neighbour needs v within that of a rounding boundary.
# Started from SMALL_CAPS' 2 % and kept there: the fp32 other-order restatement (tests/test_adapter_model.py,
# `python -m tests.test_adapter_model`; table in docs/findings/adapter_contract.md section 2) uses at most 0.0002 of a tensor over
# all eight geometries, both draws and both builds (fp16: Vs_qkv of the order-5 geometry (5, 40, 5, 17); bf16: Vs_fc2 of the order-2
# geometry; every other matrix 0.0001 or none), a hundredth of it; never fitted to a device.
ADAPTER_CAPS = {"pack": 0.02}

# The exact-dropout and order-2 kernels (oracle/exact_modes_model.py), per 16-bit output kind, under the same rule as GEMM_CAPS (the
# share is taken over the elements whose derived term is below a quarter of their own 16-bit step; one neighbour case never breaks a
# cap; a tensor with no capped element fails).  Chosen as there: the fp32 other-order restatement's largest share over all host
# cases and both builds (tests/test_exact_modes_model.py, `python -m tests.test_exact_modes_model`; table in
# docs/findings/exact_modes_contract.md section 3), doubled and rounded up to the next of 0.5 %, 1 %, 2 %; never fitted to a device.
# Measured: merge_Weff 0.0008 (fp16, Gaussian; outlier 0.0005; bf16 none) -> 0.5 %; merge_Dm 0.0005 (fp16 Gaussian and bf16 early
# training; outlier 0.0003) -> 0.5 %; dd_Dm 0.0003 (fp16; bf16 none) -> 0.5 %.  The early-training family of merge_Weff (Vs at 1e-6
# next to W at 2e-2): the delta is far below W's step, almost every element is simply W, and the restatement has NO neighbour case
# in either build; its derived term gamma(Rp + 2) (|W| + |delta|) stays below a quarter step, so the same cap is in force there, and
# where a term is not below a quarter step no cap applies (the interval alone, as for the offset LayerNorm rows).
EXACT_CAPS = {"merge_Weff": 0.005, "merge_Dm": 0.005, "dd_Dm": 0.005}

# The skinny products as stand-alone launches (oracle/skinny_model.py): T = X U, its transpose and G' = dY Vs, one kind "T", under
# the same rule as GEMM_CAPS (the share is taken over the elements whose derived term is below a quarter of their own 16-bit step; one
# neighbour case never breaks a cap).  Started from GEMM_CAPS["T"] and kept there: the fp32 other-order restatement
# (tests/test_skinny_model.py, `python -m tests.test_skinny_model`; table in docs/findings/skinny_contract.md section 3) has at most
# ONE neighbour case per tensor on every host case and in both builds, a share of at most 0.0003 (fp16; bf16 none): an eighth of half
# the cap.  A tensor of fewer than 400 elements (M = 1: 32) cannot express half the cap -- one element of it is
# more -- and is held to "at most one neighbour case", as check_16 holds it.  Never fitted to a device.
SKINNY_CAPS = {"T": GEMM_CAPS["T"]}
