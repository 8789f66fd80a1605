"""Classical-logic benchmarks (forest/benchmarking/classical_logic): the ripple-carry adder's circuit, its simulated
acquisition and the analysis of its measured shots."""
from . import primitives, reversible  # noqa: F401
from .ripple_carry_adder import (adder_expected_bits, get_success_probabilities_from_results,  # noqa: F401
                                 get_error_hamming_distributions_from_results, get_success_probabilities_from_results_batch,
                                 get_error_hamming_distributions_from_results_batch, assign_registers_to_line_or_cycle,
                                 get_qubit_registers_for_adder, adder, default_adder_registers, simulate_n_bit_adder_results,
                                 simulate_adder_statistics_batch, predicted_adder_statistics)
