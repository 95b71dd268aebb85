// oracle/standin/sdsl/int_vector.hpp -- STAND-IN, TEST INFRASTRUCTURE ONLY: empty on purpose.  The reference's miBF headers include
// this name; nothing they use comes from it (see sdsl/bit_vector_il.hpp and google/dense_hash_set beside it).
