// k_long_extend for teams of 4 lanes per wave: plain, band controls, band controls + clipping, each persistent or not
#include "gc_long_extend.hpp"
GC_LONG_EXTEND_TEAM(4)
