// tests/compat_init: an Initializer with the members compat/Initializer_ransac.inl touches -- mvKeys1, mvKeys2, mvMatches12,
// mvSets, mSigma, mMaxIterations, with the reference's types (include/Initializer.h:46, :311-338) -- and one member function,
// HF, whose body is the part of Initialize around the fragment: the locals the reference declares (:196-200), the fragment in
// place of the two threads and their joins, and RH as :220 computes it.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>
#include <opencv2/core/core.hpp>
#include "orbx.h"
namespace ORB_SLAM2 {
using namespace std;
class Initializer {
    typedef pair<int, int> Match;
public:
    Initializer(float sigma, int iterations) : mSigma(sigma), mSigma2(sigma * sigma), mMaxIterations(iterations) {}
    // what Initialize holds when the joins return, and RH
    void HF(vector<bool> &vbMatchesInliersH_out, float &SH_out, cv::Mat &H_out, vector<bool> &vbMatchesInliersF_out, float &SF_out,
            cv::Mat &F_out, float &RH_out) {
        vector<bool> vbMatchesInliersH, vbMatchesInliersF;
        float SH, SF;
        cv::Mat H, F;
#include "Initializer_ransac.inl"
        float RH = SH / (SH + SF);
        vbMatchesInliersH_out = vbMatchesInliersH; vbMatchesInliersF_out = vbMatchesInliersF;
        SH_out = SH; SF_out = SF; H_out = H; F_out = F; RH_out = RH;
    }
    vector<cv::KeyPoint> mvKeys1;
    vector<cv::KeyPoint> mvKeys2;
    vector<Match> mvMatches12;
    float mSigma, mSigma2;
    int mMaxIterations;
    vector<vector<size_t>> mvSets;
};
}  // namespace ORB_SLAM2
