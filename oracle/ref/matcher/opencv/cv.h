// oracle/ref/matcher: the reference includes <opencv/cv.h> for names that core.hpp of the stand-in already declares
