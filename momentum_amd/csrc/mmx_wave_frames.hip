// mmx_wave_frames.hip -- the frame-sequence instantiations of the one-wavefront solve: waveSolveKernel<16 / 32, true> behind
// launchWaveFrames (mmx_solve_frames).  The kernel is mmx_wave.hip's, everything frame-specific there sits under
// `if constexpr (kFrames)`; a translation unit of its own so that the two instantiations mmx_solve launches are compiled as
// they always were, and the four compile side by side.
#define MMX_WAVE_FRAMES_UNIT
#include "mmx_wave.hip"
