// oracle/ref/extractor: the reference includes this header for the cv:: names of include/ORBextractor.h; the stand-in declares all of its cv:: in one file
#pragma once
#include "../opencv2/core/core.hpp"
