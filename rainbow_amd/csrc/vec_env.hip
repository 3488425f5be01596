// vec_env.hip — device-resident vectorised environments (rb_catch_*): the whole unit is vec_env.h.
#include "vec_env.h"
