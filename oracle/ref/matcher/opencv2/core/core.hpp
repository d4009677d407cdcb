// oracle/ref/matcher: <opencv2/core/core.hpp> for compiling the reference's src/ORBmatcher.cc and src/MapPoint.cc unmodified.
// It is the cv::Mat stand-in of tests/compat_runtime/ (one file, shared: the arithmetic rule is written at its top), after the
// standard headers and the `using namespace std` that the reference's own headers pull in and its sources rely on.
#pragma once
#include <cassert>
#include <climits>
#include <cmath>
#include <list>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>
#include "../../../../../tests/compat_runtime/opencv2/core/core.hpp"
using namespace std;
