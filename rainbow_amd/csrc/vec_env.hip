// vec_env.hip — device-resident vectorised environments (rb_catch_*: vec_env.h; rb_breakout_*: breakout_env.h) and the
// environment-independent recorder of their episode returns (rb_tally_*: episode_tally.h).
#include "vec_env.h"
#include "breakout_env.h"
#include "episode_tally.h"
