// tests/compat_kfdb: the one member of ORB_SLAM2::ORBVocabulary (DBoW2::TemplatedVocabulary) compat/KeyFrameDatabase.h touches,
// and DBoW2::BowVector as the std::map it is (Thirdparty/DBoW2/DBoW2/BowVector.h).
#pragma once
#include <map>
namespace DBoW2 {
typedef unsigned int WordId;
typedef double WordValue;
class BowVector : public std::map<WordId, WordValue> {};
enum ScoringType { L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT };
}  // namespace DBoW2
namespace ORB_SLAM2 {
class ORBVocabulary {
public:
    explicit ORBVocabulary(DBoW2::ScoringType s = DBoW2::L1_NORM) : scoring_(s) {}
    DBoW2::ScoringType getScoringType() const { return scoring_; }
private:
    DBoW2::ScoringType scoring_;
};
}  // namespace ORB_SLAM2
