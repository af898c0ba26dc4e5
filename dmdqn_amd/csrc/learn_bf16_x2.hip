// learn_bf16_x2.hip -- the paired learn (dmdqn_learn_pair, k_learn_bf16_x2) of
// the bf16 instantiation of learn_h16.hpp: two consecutive learns of every
// agent in one launch.  A file of its own for its compile flags (build.py
// PER_FILE; learn_h16.hpp says why at the kernel).
#define DMDQN_H16_BF16 1
#define DMDQN_H16_PAIR 1
#include "learn_h16.hpp"
