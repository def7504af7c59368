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


def logits_ok(r_ref: float, r_model: float) -> bool:
    return r_ref <= LOGITS_ABS and r_ref <= LOGITS_VS_MODEL * max(r_model, MODEL_FLOOR)
