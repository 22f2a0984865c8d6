// G.711 a-law / mu-law expansion of the `ctucopy` executable's -format_in alaw|mulaw decoders.
// Kept in a header of its own so that tests can compile it stand-alone against the reference's table
// (oracle/_ref/libref_amulaw.so, tests/test_host_decoders.py).  The expansion itself is the one host statement of it, wire_g711
// (csrc/wire_layout.h), which ctu_wire_expand and the pipe's byte accumulator read too.
#pragma once
#include <cstdint>

#include "../csrc/wire_layout.h"

inline int16_t g711_to_linear(uint8_t code, bool alaw) { return wire_g711(code, alaw); }
