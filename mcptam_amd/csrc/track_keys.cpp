// The keyed shuffle of mcp_track_map (include/mcp_img.h: mcp_mix64, mcp_track_shuffle_key) as exported functions, for callers that do not
// compile the header (ctypes).  This file does not include the header, whose definitions are static inline; the bodies are the same.
#include <stdint.h>

extern "C" {
uint64_t mcp_mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31);
}
uint64_t mcp_track_shuffle_key(uint64_t seed, int stage, int cam, int row) {
  return mcp_mix64(mcp_mix64(seed ^ ((uint64_t)stage << 40) ^ ((uint64_t)cam << 32)) ^ (uint32_t)row);
}
}
