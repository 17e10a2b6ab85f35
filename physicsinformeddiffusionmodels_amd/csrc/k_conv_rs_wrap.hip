// The circular-padding half of the row-streaming 3x3 convolution: conv3x3_rs_kernel<NCH, NT, RM, BNP, true> and launch_conv_rs_wrap,
// which launch_conv_rs (k_conv_rs.hip) hands every wrapping geometry (ConvGeom::wrap).  The kernel template and the launcher are
// k_conv_rs.hip's own text - one source, two translation units, so that the instantiations of the two padding modes compile
// side by side.
#define PIDM_CONV_RS_WRAP_TU 1
#include "k_conv_rs.hip"
