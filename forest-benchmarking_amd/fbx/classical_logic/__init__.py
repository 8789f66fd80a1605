"""Analysis of classical-logic benchmarks (forest/benchmarking/classical_logic) from measured shots."""
from .ripple_carry_adder import (adder_expected_bits, get_success_probabilities_from_results,  # noqa: F401
                                 get_error_hamming_distributions_from_results, get_success_probabilities_from_results_batch,
                                 get_error_hamming_distributions_from_results_batch)
