// pairing kernels (Miller loop, Fp12 product tree, final exponentiation with comparison) for bls381 (explicit instantiation; see pairing_impl.hpp)
#include "pairing_impl.hpp"
CG_INSTANTIATE_PAIRING(Bls381Pairing)
