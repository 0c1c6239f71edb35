"""Import-name shim: lets existing callers keep `from sparse_matrix_mult import
sparse_matrix_multiply` (reference sparse_matrix_mult/__init__.py:1-3) while the work is done
by sparse_matrix_mult_amd on the GPU."""
from sparse_matrix_mult_amd.matrix_ops import (KroneckerOperand, PinnedOperand, VariogramResult, covariance_on_pattern, empirical_variogram, innovation_solve, innovation_logdet, interpolation_operator,
                                               kronecker_product, localization_taper,
                                               masked_matrix_multiply, pin_operand,
                                               sampled_dense_product, sparse_dense_multiply, sparse_matrix_multiply,
                                               sparse_triple_product, triple_product_apply)

__all__ = ['sparse_matrix_multiply', 'sparse_triple_product', 'masked_matrix_multiply', 'sparse_dense_multiply',
           'triple_product_apply', 'innovation_solve', 'innovation_logdet', 'sampled_dense_product', 'localization_taper', 'pin_operand',
           'PinnedOperand', 'kronecker_product', 'KroneckerOperand', 'interpolation_operator', 'covariance_on_pattern',
           'empirical_variogram', 'VariogramResult']
