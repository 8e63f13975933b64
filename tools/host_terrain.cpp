// host_terrain.cpp -- TEST TOOL, not product code.
// host_terrain_batch lives in host_ground.cpp, beside the flat entry, in tools/libhost_ground.so.  This file keeps the library's
// former name buildable (g++ ... -o libhost_terrain.so host_terrain.cpp) for a tests/ tree from before the two were one.
#include "host_ground.cpp"
